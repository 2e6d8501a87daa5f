"""The worker loop of videosd_amd.dispatch, pinned call by call without a GPU: one script of requests (every message, the final None
included, queued in the pipe before the loop starts, so nothing depends on timing) against three recording stand-ins; the full trace of
what the pipeline was asked and the exact sequence of replies are compared with literals derived from the loop's rules:

  * an `infer` takes the queued `infer` calls behind it whose options are the same (per-frame values apart, within one option class)
    into ONE launch, up to `max_batch`; the launch gets the per-frame values as lists in request order (a missing one: `infer`'s default);
  * anything else that is next (other options, another method, shutdown) is served next and ends the batch;
  * a launch goes on the LOWEST free lane, beside what is in flight (after `needs_idle` was asked when its options differ from the
    newest launch in flight; a pipeline that says yes is drained first); when every lane is busy the oldest launch is handed back;
  * `__metrics__` answers between frames without a drain; any other method drains and runs alone; a launch that raises drains, fails
    its requests with (type name, text) and the loop goes on; `can_batch` false: alone, through `infer`; shutdown drains."""
import multiprocessing as mp
import os
import sys
import threading

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from helpers_fake_pipeline import FakePipeline  # noqa: E402

TRACE = []
DEFAULT_PROMPT = ["pixar, cg"]


class _Recorder(FakePipeline):
    """logs every call the worker loop makes; a result's first pixel says (frames in its launch, lane or 255, 0)"""

    def _out(self, imgs, opts, lane):
        outs = []
        for img in imgs:
            a = 255 - np.asarray(img.convert("RGB").resize((opts.get("width", 640), opts.get("height", 360))))
            a[0, 0] = (len(imgs), 255 if lane is None else lane, 0)
            outs.append(Image.fromarray(a.astype(np.uint8), "RGB"))
        return outs

    @staticmethod
    def _check(opts):
        if opts.get("steps") == 13:
            raise ValueError("steps 13")

    def can_batch(self, **opts):
        TRACE.append(("can_batch", opts))
        return not opts.get("ref")

    def infer(self, img, **opts):
        TRACE.append(("infer", None, 1, opts))
        self._check(opts)
        return self._out([img], opts, None)[0]

    def infer_batch(self, imgs, **opts):
        TRACE.append(("infer_batch", None, len(imgs), opts))
        self._check(opts)
        return self._out(imgs, opts, None)

    def ping(self, x):
        TRACE.append(("ping", x))
        return 2 * x


class InferBatchOnly(_Recorder):
    """(b): all three per-frame attributes, `option_class`, `needs_idle` -- and no two-phase launch"""
    per_frame_seed = per_frame_prompt = per_frame_options = True
    submit_batch = collect_batch = property()  # (hasattr is False)

    def option_class(self, options):
        TRACE.append(("option_class", options))
        return 1 if options.get("strength", 0.4) < 0.1 else 2

    def needs_idle(self, **opts):
        TRACE.append(("needs_idle", opts))
        return bool(opts.get("idle"))


class TwoPhase(InferBatchOnly):
    """(a) and (c): the same with `submit_batch` / `collect_batch`"""

    def submit_batch(self, imgs, lane=0, **opts):
        TRACE.append(("submit_batch", lane, len(imgs), opts))
        self._check(opts)
        return ([im.copy() for im in imgs], opts, lane)

    def collect_batch(self, handle):
        imgs, opts, lane = handle
        TRACE.append(("collect_batch", lane, len(imgs)))
        return self._out(imgs, opts, lane)


H = dict(height=12, width=16)
SMALL = dict(height=6, width=8)
SCRIPT = [
    ("infer", dict(H, steps=2, seed=100, prompt="a cat", strength=0.6, controlnet_scale=1.5)),  # 0 \
    ("infer", dict(H, steps=2, seed=101, prompt="a dog", strength=0.9)),                        # 1  > one option class, all else equal
    ("infer", dict(H, steps=2, prompt=["a cat"], strength=0.3, controlnet_scale=0.5)),          # 2 /
    ("infer", dict(SMALL, steps=2, seed=103)),                                                  # 3 another size
    ("infer", dict(H, steps=2, seed=104, strength=0.02)),                                       # 4 another option class (and size)
    ("__metrics__", None),                                                                      # 5
    ("infer", dict(H, steps=2, seed=106, strength=0.03)),                                       # 6 the class of 4, which is in flight
    ("infer", dict(H, steps=2, seed=107, strength=0.6)),                                        # 7 the other class again
    ("ping", 5),                                                                                # 8 an arbitrary method
    ("infer", dict(H, steps=2, seed=109)),                                                      # 9
    ("infer", dict(SMALL, steps=2, seed=110, idle=True)),                                       # 10 the pipeline asks for a drain
    ("infer", dict(H, steps=13, seed=111)),                                                     # 11 the launch raises ValueError
    ("infer", dict(H, steps=2, seed=112, ref=True)),                                            # 12 `can_batch` is false
    ("__metrics__", None),                                                                      # 13
    ("infer", dict(H, steps=4, seed=114)),                                                      # 14 \ in flight at shutdown
    ("infer", dict(H, steps=4, seed=115, strength=0.7)),                                        # 15 /
]


def K(rid):
    return dict(SCRIPT[rid][1])


def L(rid, seed, prompts, strength, scale):
    """the kwargs of a launch whose first request is `rid`: its options, the per-frame values as lists"""
    return dict(K(rid), seed=seed, prompts=prompts, strength=strength, controlnet_scale=scale)


def L1(rid):
    k = K(rid)
    return L(rid, [k.get("seed", 42)], [k.get("prompt", DEFAULT_PROMPT)], [k.get("strength", 0.4)], [k.get("controlnet_scale", 1)])


def _serve(factory, max_batch, lanes):
    """the worker loop in a thread of this process, the whole script ALREADY queued when it starts -> (trace, replies in order)"""
    from videosd_amd.dispatch import _worker_main

    del TRACE[:]
    parent, child = mp.Pipe()
    for rid, (method, what) in enumerate(SCRIPT):
        if method == "infer":
            img = Image.fromarray(np.full((12, 16, 3), 10 * (rid + 1), np.uint8), "RGB")
            parent.send((rid, "infer", (img,), what))
        else:
            parent.send((rid, method, () if what is None else (what,), {}))
    parent.send(None)
    t = threading.Thread(target=_worker_main, args=(child, factory, dict(model="m", controlnet="c", device=0)),
                         kwargs=dict(max_batch=max_batch, lanes=lanes))
    t.start()
    t.join(60)
    assert not t.is_alive()
    assert parent.recv() == ("ready", None)
    replies = []
    while parent.poll(0):
        rid, ok, payload = parent.recv()
        if isinstance(payload, Image.Image):
            a = np.asarray(payload)
            payload = ("img", payload.size, tuple(int(v) for v in a[0, 0]), int(a[1, 1, 0]))
        elif isinstance(payload, dict):  # metrics: the counts, and that every key is there
            assert set(payload) == {"frames", "launches", "errors", "uptime_s", "fps", "p50_ms", "p95_ms", "frames_per_launch", "rank", "world",
                                    "device", "pid"}, sorted(payload)
            payload = ("metrics",) + tuple(payload[k] for k in ("frames", "launches", "errors", "rank", "world", "device"))
        replies.append((rid, ok, payload))
    return list(TRACE), replies


def img(rid, size, n, lane):
    """the reply to `infer` request rid: its own frame (inverted), out of a launch of n on `lane`"""
    return (rid, True, ("img", size, (n, 255 if lane is None else lane, 0), 255 - 10 * (rid + 1)))


BIG, LITTLE = (16, 12), (8, 6)
FIRST3 = L(0, [100, 101, 42], ["a cat", "a dog", ["a cat"]], [0.6, 0.9, 0.3], [1.5, 1, 0.5])
LAST2 = L(14, [114, 115], [DEFAULT_PROMPT, DEFAULT_PROMPT], [0.4, 0.7], [1, 1])
FAILED = (11, False, ("ValueError", "steps 13"))
METRICS_END = (13, True, ("metrics", 10, 8, 1, 0, 1, 0))  # 10 frames answered in 8 launches; the failed request is the one error


def test_two_lanes_batches_of_three():
    trace, replies = _serve("test_worker_trace_host:TwoPhase", max_batch=3, lanes=2)
    oc, ni, cb = (lambda r: ("option_class", K(r))), (lambda r: ("needs_idle", K(r))), (lambda r: ("can_batch", K(r)))
    assert trace == [
        # 0 takes 1 and 2 (each compared with the FIRST request: other values, one class); the batch is full, 3 stays in the pipe
        cb(0), oc(1), oc(0), oc(2), oc(0), ("submit_batch", 0, 3, FIRST3),
        # 3: another size ends at once against 4 (no class is asked: other options differ); it goes BESIDE the launch in flight, lane 1;
        # both lanes busy: the oldest comes back
        cb(3), ni(3), ("submit_batch", 1, 1, L1(3)), ("collect_batch", 0, 3),
        # 4: __metrics__ is next -> the batch ends; lane 0 is the lowest free one
        cb(4), ni(4), ("submit_batch", 0, 1, L1(4)), ("collect_batch", 1, 1),
        # (5: __metrics__ touches neither the pipeline nor the launch of 4)
        # 6: 7 is of the other class -> served next; 6 is of the class in flight (4): no `needs_idle`
        cb(6), oc(7), oc(6), oc(4), oc(6), ("submit_batch", 1, 1, L1(6)), ("collect_batch", 0, 1),
        # 7: the class differs from the launch in flight (6): the pipeline is asked, and need not idle
        cb(7), oc(6), oc(7), ni(7), ("submit_batch", 0, 1, L1(7)), ("collect_batch", 1, 1),
        # 8: an arbitrary method drains, then runs alone
        ("collect_batch", 0, 1), ("ping", 5),
        # 9 on an idle worker: lane 0; 10 makes the pipeline ask for a drain: 9 is collected first, 10 lands on lane 0 again
        cb(9), ("submit_batch", 0, 1, L1(9)),
        cb(10), ni(10), ("collect_batch", 0, 1), ("submit_batch", 0, 1, L1(10)),
        # 11: its launch raises: what is in flight is drained, then 11 fails
        cb(11), ni(11), ("submit_batch", 1, 1, L1(11)), ("collect_batch", 0, 1),
        # 12: `can_batch` is false: alone, through `infer`, with its options as they came
        cb(12), ("infer", None, 1, K(12)),
        # 14 takes 15; shutdown is next: the launch is collected on the way out
        cb(14), oc(15), oc(14), ("submit_batch", 0, 2, LAST2), ("collect_batch", 0, 2),
    ]
    assert replies == [
        img(0, BIG, 3, 0), img(1, BIG, 3, 0), img(2, BIG, 3, 0), img(3, LITTLE, 1, 1),
        (5, True, ("metrics", 4, 2, 0, 0, 1, 0)),  # 4's launch is still in flight
        img(4, BIG, 1, 0), img(6, BIG, 1, 1), img(7, BIG, 1, 0), (8, True, 10), img(9, BIG, 1, 0), img(10, LITTLE, 1, 0), FAILED,
        img(12, BIG, 1, None), METRICS_END, img(14, BIG, 2, 0), img(15, BIG, 2, 0),
    ]


def test_without_the_two_phase_launch_batches_go_through_infer_batch():
    trace, replies = _serve("test_worker_trace_host:InferBatchOnly", max_batch=3, lanes=2)
    oc, cb = (lambda r: ("option_class", K(r))), (lambda r: ("can_batch", K(r)))
    one = lambda r: [cb(r), ("infer", None, 1, K(r))]  # noqa: E731  (a batch of one goes through `infer`, its options as they came)
    assert trace == [
        cb(0), oc(1), oc(0), oc(2), oc(0), ("infer_batch", None, 3, FIRST3),
        *one(3), *one(4),
        cb(6), oc(7), oc(6), ("infer", None, 1, K(6)),  # (nothing is ever in flight: the only comparisons are those of coalescing)
        *one(7), ("ping", 5), *one(9), *one(10), *one(11), *one(12),
        cb(14), oc(15), oc(14), ("infer_batch", None, 2, LAST2),
    ]
    assert replies == [
        img(0, BIG, 3, None), img(1, BIG, 3, None), img(2, BIG, 3, None), img(3, LITTLE, 1, None), img(4, BIG, 1, None),
        (5, True, ("metrics", 5, 3, 0, 0, 1, 0)),
        img(6, BIG, 1, None), img(7, BIG, 1, None), (8, True, 10), img(9, BIG, 1, None), img(10, LITTLE, 1, None), FAILED,
        img(12, BIG, 1, None), METRICS_END, img(14, BIG, 2, None), img(15, BIG, 2, None),
    ]


def test_max_batch_one_serves_every_call_alone_in_order():
    trace, replies = _serve("test_worker_trace_host:TwoPhase", max_batch=1, lanes=2)
    infers = [r for r, (m, _w) in enumerate(SCRIPT) if m == "infer"]
    want = [("infer", None, 1, K(r)) for r in infers]  # never `can_batch`, never a class, never a lane
    want.insert(infers.index(9), ("ping", 5))
    assert trace == want
    assert replies == [
        img(0, BIG, 1, None), img(1, BIG, 1, None), img(2, BIG, 1, None), img(3, LITTLE, 1, None), img(4, BIG, 1, None),
        (5, True, ("metrics", 5, 5, 0, 0, 1, 0)),
        img(6, BIG, 1, None), img(7, BIG, 1, None), (8, True, 10), img(9, BIG, 1, None), img(10, LITTLE, 1, None), FAILED,
        img(12, BIG, 1, None), (13, True, ("metrics", 10, 10, 1, 0, 1, 0)), img(14, BIG, 1, None), img(15, BIG, 1, None),
    ]
