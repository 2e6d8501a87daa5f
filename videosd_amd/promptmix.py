"""The canonical form of a prompt MIX (include/vsd.h THE PROMPT MIX): what `prompt` may be besides a text, stated once as pure functions
with no torch or device imports, so that the class (pipeline.py), the worker and the dispatcher (dispatch.py) agree on what two
spellings of one mix are, and the rules are tested on the host (tests/test_prompt_mix_host.py).

A caller writes a mix as JSON-able data, `{"mix": [["text a", 0.3], ["text b", 0.7]]}`: 1 to 4 texts with weights that are finite and
not negative, at least one of them positive.  `canonical` brings it to ONE form:
  * texts that repeat are merged, their weights added (in fp64, in the order written);
  * components of weight zero are dropped;
  * the rest is ordered by text, so that equal mixes give equal keys and equal bits whatever order the caller wrote them in;
  * every weight becomes fp32(w / sum) with the quotient taken in fp64: the weights the device multiplies by;
  * a mix that comes down to one component IS that prompt: `canonical` returns the text, and with it the same cache key, the same code
    path and the same bits as the plain prompt.
Anything that is not a dict is a plain prompt and passes through unchanged."""
import math
import struct
from typing import NamedTuple, Tuple

MAX_COMPONENTS = 4  # (the sources and weights of vsd_prompt_mix travel as launch arguments)


class Mix(NamedTuple):
    """A canonical mix of two to MAX_COMPONENTS prompts: ((text, weight), ...) ordered by text, the weights fp32 values that sum to 1 up
    to fp32 rounding.  Hashable, comparable and picklable: it is its own cache key."""
    components: Tuple[Tuple[str, float], ...]

    @property
    def texts(self):
        return tuple(t for t, _w in self.components)

    @property
    def weights(self):
        return tuple(w for _t, w in self.components)


def fp32(x: float) -> float:
    """the fp32 value nearest to x (ties to even), as a Python float"""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def normalized(weights):
    """fp32(w_i / sum(w)), the quotient in fp64 -- the weights of a mix as the device takes them"""
    total = math.fsum(weights)
    return tuple(fp32(float(w) / total) for w in weights)


def is_mix(prompt) -> bool:
    """is `prompt` written as a mix (whatever it comes down to)?"""
    return isinstance(prompt, (dict, Mix))


def canonical(prompt):
    """`prompt` as `infer` takes it -> a plain prompt unchanged, the text of a mix that comes down to one component, or a `Mix`.
    ValueError, naming what is wrong, for a dict that is not a mix as described above."""
    if isinstance(prompt, Mix) or not isinstance(prompt, dict):
        return prompt
    if "mix" not in prompt:
        raise ValueError(f'prompt: a dict must be a mix, {{"mix": [[text, weight], ...]}}; this one has the keys {sorted(map(str, prompt))}')
    if len(prompt) != 1:
        raise ValueError(f'prompt: a mix is a dict with the one key "mix"; this one also has {sorted(str(k) for k in prompt if k != "mix")}')
    try:
        pairs = [tuple(c) for c in prompt["mix"]]
    except TypeError:
        raise ValueError('prompt: "mix" must be a list of [text, weight] pairs') from None
    merged = {}
    for c in pairs:
        if len(c) != 2:
            raise ValueError(f'prompt: every component of a mix is a [text, weight] pair, got {list(c)!r}')
        text, w = c
        if not isinstance(text, str):
            raise ValueError(f"prompt: the text of a mix component must be a string, got {type(text).__name__} ({text!r})")
        if isinstance(w, bool) or not isinstance(w, (int, float)):
            raise ValueError(f"prompt: the weight of {text!r} must be a number, got {type(w).__name__}")
        w = float(w)
        if not math.isfinite(w):
            raise ValueError(f"prompt: the weight of {text!r} is not finite ({w})")
        if w < 0:
            raise ValueError(f"prompt: the weight of {text!r} is negative ({w}); a mix is a convex combination")
        merged[text] = merged.get(text, 0.0) + w
    live = sorted((t, w) for t, w in merged.items() if w > 0)
    if not live:
        raise ValueError("prompt: a mix needs at least one component with a positive weight")
    if not math.isfinite(math.fsum(w for _t, w in live)):
        raise ValueError("prompt: the weights of the mix do not have a finite sum")
    if len(live) > MAX_COMPONENTS:
        raise ValueError(f"prompt: a mix has at most {MAX_COMPONENTS} components, this one has {len(live)} after merging")
    if len(live) == 1:
        return live[0][0]
    ws = normalized([w for _t, w in live])
    live = [(t, w) for (t, _w), w in zip(live, ws) if w > 0]  # (a weight that fp32 rounds to zero beside the others)
    if len(live) == 1:
        return live[0][0]
    return Mix(tuple(live))


def prompt_key(prompt):
    """What the prompt caches (and an SDXL plan, and the dispatcher's bookkeeping) know a prompt by: the string, the list as a tuple (the
    reference's default is a one-element list), or the canonical `Mix`."""
    p = canonical(prompt)
    return p if isinstance(p, (str, Mix)) else tuple(p)


def component_prompts(prompt):
    """the prompts a worker must hold in its cache to run `prompt`: the texts of a mix, else the prompt itself"""
    p = canonical(prompt)
    return list(p.texts) if isinstance(p, Mix) else [p]
