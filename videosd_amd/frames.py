"""Planar YUV 4:2:0 frames ("I420", PyAV's `yuv420p`): what a decoded WebRTC frame is and what its encoder takes.

`I420Frame` is the product's own container for one: a single contiguous uint8 buffer with `y`, `u`, `v` views.  It is built from
an `av.VideoFrame` by duck typing (`from_av`) -- this package never imports `av` -- and goes back through `to_ndarray()`, the array
`av.VideoFrame.from_ndarray(a, format="yuv420p")` takes.  The colour contract (8-bit BT.601 studio range, integer form, no chroma
interpolation) is stated in include/vsd.h; `to_rgb` / `from_rgb` are the library's host loops of it (no GPU needed), the kernels of
csrc/yuv.hip give the same bytes.  How far libswscale's conversion is from this contract is not measured.
"""
import numpy as np

# what the contract does not cover is refused by name, never approximated
UNSUPPORTED = {
    "yuvj420p": "full-range (JPEG) 4:2:0: the contract is studio range (Y 16..235)",
    "nv12": "semi-planar chroma", "nv21": "semi-planar chroma",
    "yuv422p": "4:2:2", "yuvj422p": "4:2:2", "yuv444p": "4:4:4", "yuvj444p": "4:4:4",
    "yuv420p10le": "more than 8 bits", "yuv420p10be": "more than 8 bits", "yuv420p12le": "more than 8 bits", "p010le": "more than 8 bits",
}


def chroma_shape(height: int, width: int):
    return (int(height) + 1) // 2, (int(width) + 1) // 2


def _format_name(frame):
    fmt = getattr(frame, "format", None)
    return getattr(fmt, "name", None)


def is_av_like(obj) -> bool:
    """Does `obj` look like an av.VideoFrame (of ANY pixel format)?  `format.name`, `width`, `height` and `planes`."""
    return isinstance(_format_name(obj), str) and hasattr(obj, "planes") and hasattr(obj, "width") and hasattr(obj, "height")


def is_i420(obj) -> bool:
    """An `I420Frame`, or an object `I420Frame.from_av` is meant for (which may still refuse its pixel format, with a reason)."""
    return isinstance(obj, I420Frame) or is_av_like(obj)


def av_plane_views(frame):
    """(y, u, v) of a yuv420p av-like frame as read-only 2-D views of its planes' own memory (rows `line_size` bytes apart); raises
    ValueError for another pixel format (by name, with the reason) or a plane too short for its rows.  Nothing is copied."""
    name = _format_name(frame)
    if name != "yuv420p":
        why = UNSUPPORTED.get(name, "not 8-bit planar 4:2:0")
        raise ValueError(f"pixel format {name!r} is not supported ({why}); only yuv420p (8-bit BT.601 studio range) is -- reformat the "
                         "frame first")
    w, h = int(frame.width), int(frame.height)
    planes = list(frame.planes)
    if w < 1 or h < 1 or len(planes) < 3:
        raise ValueError(f"a yuv420p frame has three planes and non-zero sides, got {len(planes)} plane(s), {w} x {h}")
    views = []
    for pl, (rows, cols) in zip(planes[:3], ((h, w), chroma_shape(h, w), chroma_shape(h, w))):
        ls = int(pl.line_size)
        raw = np.frombuffer(pl, dtype=np.uint8)
        if ls < cols or raw.size < (rows - 1) * ls + cols:
            raise ValueError(f"a plane of {raw.size} bytes with line_size {ls} does not hold {rows} rows of {cols} bytes")
        views.append(np.lib.stride_tricks.as_strided(raw, shape=(rows, cols), strides=(ls, 1), writeable=False))
    return tuple(views)


def _lib():
    from . import lib as L

    return L.load()


class I420Frame:
    """One 8-bit planar 4:2:0 frame: `data` (uint8, height * width + 2 * ceil(height / 2) * ceil(width / 2) bytes: Y, then U, then V, rows
    tight), `y` / `u` / `v` views of it, `width`, `height`.  Odd sizes are legal (chroma planes round up)."""

    __slots__ = ("data", "width", "height")

    def __init__(self, data, width: int, height: int):
        width, height = int(width), int(height)
        if width < 1 or height < 1:
            raise ValueError(f"I420Frame: {width} x {height}: both sides must be at least 1")
        a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if a.dtype != np.uint8 or a.ndim != 1 or a.size != self.nbytes_for(width, height) or not a.flags.c_contiguous:
            raise ValueError(f"I420Frame: a {width} x {height} frame is {self.nbytes_for(width, height)} contiguous uint8 bytes, got "
                             f"{a.dtype} {a.shape}")
        self.data, self.width, self.height = a, width, height

    @staticmethod
    def nbytes_for(width: int, height: int) -> int:
        ch, cw = chroma_shape(height, width)
        return int(height) * int(width) + 2 * ch * cw

    @classmethod
    def empty(cls, width: int, height: int) -> "I420Frame":
        return cls(np.empty(cls.nbytes_for(width, height), np.uint8), width, height)

    @property
    def size(self):
        """(width, height), as PIL's `Image.size`"""
        return self.width, self.height

    @property
    def y(self) -> np.ndarray:
        return self.data[:self.height * self.width].reshape(self.height, self.width)

    @property
    def u(self) -> np.ndarray:
        ch, cw = chroma_shape(self.height, self.width)
        o = self.height * self.width
        return self.data[o:o + ch * cw].reshape(ch, cw)

    @property
    def v(self) -> np.ndarray:
        ch, cw = chroma_shape(self.height, self.width)
        o = self.height * self.width + ch * cw
        return self.data[o:o + ch * cw].reshape(ch, cw)

    # ---- construction
    @classmethod
    def from_planes(cls, y, u, v) -> "I420Frame":
        """Three uint8 2-D arrays with any strides (views of padded rows included), copied tight."""
        y, u, v = (np.asarray(p) for p in (y, u, v))
        if any(p.dtype != np.uint8 or p.ndim != 2 for p in (y, u, v)) or y.size == 0:
            raise ValueError("I420Frame.from_planes: three non-empty uint8 2-D arrays (8-bit planar 4:2:0)")
        h, w = y.shape
        if u.shape != chroma_shape(h, w) or v.shape != u.shape:
            raise ValueError(f"I420Frame.from_planes: a {w} x {h} luma plane goes with chroma planes of {chroma_shape(h, w)[::-1]} (4:2:0), got "
                             f"{u.shape[::-1]} and {v.shape[::-1]}")
        f = cls.empty(w, h)
        f.y[...] = y
        f.u[...] = u
        f.v[...] = v
        return f

    @classmethod
    def from_av(cls, frame) -> "I420Frame":
        """From an av.VideoFrame, by what PyAV exposes and without importing it: `format.name == "yuv420p"`, `width`, `height`,
        `planes[i]` with `.line_size` and the buffer protocol.  Every other pixel format is refused with a reason."""
        if isinstance(frame, cls):
            return frame
        return cls.from_planes(*av_plane_views(frame))

    @classmethod
    def coerce(cls, obj) -> "I420Frame":
        return obj if isinstance(obj, cls) else cls.from_av(obj)

    # ---- out
    def to_ndarray(self) -> np.ndarray:
        """The (height * 3 / 2, width) uint8 array `av.VideoFrame.from_ndarray(a, format="yuv420p")` takes (a view of `data`); even sizes only."""
        if (self.width | self.height) & 1:
            raise ValueError(f"I420Frame.to_ndarray: {self.width} x {self.height}: the (h * 3 / 2, w) layout needs even sides")
        return self.data.reshape(self.height * 3 // 2, self.width)

    def to_rgb(self) -> np.ndarray:
        """uint8 [height][width][3] by the library's host loop of the colour contract (include/vsd.h vsd_i420_to_rgb_host)"""
        out = np.empty((self.height, self.width, 3), np.uint8)
        y, u, v = self.y, self.u, self.v
        rc = _lib().vsd_i420_to_rgb_host(y.ctypes.data, y.strides[0], u.ctypes.data, v.ctypes.data, u.strides[0], 0, 0, self.height, self.width,
                                         out.ctypes.data, 3 * self.width)
        if rc != 0:
            raise ValueError(f"vsd_i420_to_rgb_host refused a {self.width} x {self.height} frame ({rc})")
        return out

    @classmethod
    def from_rgb(cls, rgb) -> "I420Frame":
        """From uint8 [height][width][3] (or a PIL RGB image) with even sides, by the host loop of the contract (vsd_rgb_to_i420_host)"""
        a = np.asarray(rgb)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"I420Frame.from_rgb: uint8 [h][w][3], got {a.dtype} {a.shape}")
        h, w = a.shape[:2]
        if h < 1 or w < 1 or (h | w) & 1:
            raise ValueError(f"I420Frame.from_rgb: {w} x {h}: 4:2:0 output needs even, non-zero sides")
        a = np.ascontiguousarray(a)
        f = cls.empty(w, h)
        y, u, v = f.y, f.u, f.v
        rc = _lib().vsd_rgb_to_i420_host(a.ctypes.data, h, w, y.ctypes.data, u.ctypes.data, v.ctypes.data, w, w // 2)
        if rc != 0:
            raise ValueError(f"vsd_rgb_to_i420_host refused a {w} x {h} frame ({rc})")
        return f

    # ---- value semantics
    def __reduce__(self):
        return (I420Frame, (np.array(self.data, copy=True), self.width, self.height))

    def __eq__(self, other):
        return isinstance(other, I420Frame) and self.size == other.size and np.array_equal(self.data, other.data)

    __hash__ = None

    def __repr__(self):
        return f"I420Frame({self.width} x {self.height})"


__all__ = ["I420Frame", "is_i420", "av_plane_views", "UNSUPPORTED"]
