"""How a frame crosses between the parent (dispatch.RemotePipeline) and a worker (worker._Worker) without being pickled: rings of fixed-size
shared-memory slots and ONE wire format -- a frame in a slot travels on the pipe as `(tag, slot, width, height)`, packed RGB or packed I420.
`encode_frame` / `decode_frame` / `is_slot_ref` are the only code that knows the tags.  Imports neither the GPU library nor torch."""
from contextlib import suppress
from typing import Optional

from .frames import I420Frame

SHM_RGB, SHM_I420 = "__shm__", "__shm420__"


class _ShmRing:
    """`slots` fixed-size RGB slots in one POSIX shared-memory segment.  The parent owns allocation (a free list);
    slot i of the request ring pairs with slot i of the reply ring, so a reply needs no allocation of its own."""

    def __init__(self, slots: int, slot_bytes: int, name: Optional[str] = None):
        from multiprocessing import shared_memory

        self.slots, self.slot_bytes = slots, slot_bytes
        if name is None:
            self.shm = shared_memory.SharedMemory(create=True, size=slots * slot_bytes)
            self.owner = True
        else:
            self.shm = shared_memory.SharedMemory(name=name)
            self.owner = False  # (spawned children share the parent's resource tracker: nothing to unregister here)

    def view(self, slot: int, nbytes: int) -> memoryview:
        o = slot * self.slot_bytes
        return self.shm.buf[o:o + nbytes]

    def close(self):
        # (two steps: `close` raises BufferError while a frame's memoryview is still alive -- a worker that died with frames in
        #  flight -- and the segment must lose its NAME anyway, or every respawn leaves one behind in /dev/shm until exit)
        with suppress(Exception):
            self.shm.close()
        if self.owner:
            with suppress(Exception):
                self.shm.unlink()
            self.owner = False


def is_slot_ref(x) -> bool:
    """Is `x` what `encode_frame` returns: a frame that lies in a slot?"""
    return isinstance(x, tuple) and bool(x) and x[0] in (SHM_RGB, SHM_I420)


def is_frame(x) -> bool:
    """Can `x` ride a slot: an I420Frame, or an image in PIL's terms (`tobytes`, `size`)?"""
    return isinstance(x, I420Frame) or (hasattr(x, "tobytes") and hasattr(x, "size"))


def encode_frame(ring: _ShmRing, slot: int, frame) -> Optional[tuple]:
    """`frame` into `slot` -> what goes on the pipe in its place, or None when it does not fit a slot (nothing is written then).
    A PIL image crosses as packed RGB.  An `I420Frame`, or the (y, u, v) plane views of one (`frames.av_plane_views` of an av frame:
    padded `line_size` rows read in place, once), crosses as packed I420 -- Y, U, V, rows tight: 1.5 bytes per pixel where RGB has 3;
    plane copies only, no arithmetic (numpy row copies, GIL released)."""
    import numpy as np

    if isinstance(frame, I420Frame):
        frame = (frame.y, frame.u, frame.v)
    if isinstance(frame, tuple):
        h, w = frame[0].shape
        n = I420Frame.nbytes_for(w, h)
        if n > ring.slot_bytes:
            return None
        dst = I420Frame(np.frombuffer(ring.view(slot, n), dtype=np.uint8), w, h)
        dst.y[...], dst.u[...], dst.v[...] = frame
        return (SHM_I420, slot, w, h)
    img = frame if frame.mode == "RGB" else frame.convert("RGB")
    w, h = img.size
    n = w * h * 3
    if n > ring.slot_bytes:
        return None
    # np.asarray(img) packs the pixels in one call (0.26 ms for 512x512 on the build box; `img.tobytes()` goes through the raw
    # encoder in 64 KB pieces and a join: 0.9 ms -- the largest single item of the parent's per-frame cost in
    # scripts/dispatch_ceiling.py); the copy into the slot is a numpy memcpy, which runs with the GIL released
    np.frombuffer(ring.view(slot, n), dtype=np.uint8)[:] = np.asarray(img).reshape(-1)
    return (SHM_RGB, slot, w, h)


def decode_frame(ring: _ShmRing, ref: tuple, copy: bool):
    """The frame a slot reference names: a PIL image, or an I420Frame.  copy=False: an I420Frame's planes are VIEWS of the slot (the
    worker: the request slot is held until the reply); copy=True: it owns its bytes (the parent: the reply slot is free again when
    this returns).  A PIL image owns its pixels either way: packed RGB is not Pillow's storage layout -- it keeps 4 bytes per pixel --
    so `frombuffer` DECODES the slot into storage of the image's own: one pass, with the GIL released.  (`frombytes(bytes(mv))` -- the
    first form -- copied the slot once more in front of the same decode: 0.05 ms of the parent's 0.9 ms per frame.)"""
    tag, slot, w, h = ref
    if tag == SHM_I420:
        import numpy as np

        a = np.frombuffer(ring.view(slot, I420Frame.nbytes_for(w, h)), dtype=np.uint8)
        return I420Frame(a.copy() if copy else a, w, h)
    from PIL import Image

    return Image.frombuffer("RGB", (w, h), ring.view(slot, w * h * 3), "raw", "RGB", 0, 1)
