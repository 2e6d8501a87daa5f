"""Record the bits of the scheduler kernels (include/vsd.h THE SCHEDULER ARITHMETIC) on the MI355X: tests/golden/scheduler_bits.json.

Run once against the library of the commit whose bits are to be kept (VSD_LIB selects a library; an argument another output path):
    python tests/golden/make_scheduler_bits.py [out.json]
tests/test_scheduler_bits_gpu.py imports the inputs and `run_dev` from here and holds every later build to the recorded digests.

Inputs: built by integer arithmetic alone, so every machine builds the same bits -- the Philox words of tests/seed_cases.py (numpy uint64
arithmetic) mapped to fp16 k / 2048, k a 14-bit integer in [-8192, 8192) (exact in fp32, rounded to fp16 by the IEEE conversion), and to the
fp32 noise table k * 2^-21, k a 24-bit integer in [-2^23, 2^23) (exact).  All eight channels of the fp16 inputs are filled: the kernels read
four.  No randn, no libm.
Size: hw = 2^18 + 1 latent pixels (the last workgroup is partial) x 2 images = 2.1 M values per output: a contraction of the fp32 operations
other than the contract's flips 30 to 180 fp16 results per million, so the least sensitive one is expected to change some 65 values here.
Recorded: SHA-256 of the fp16 [B * hw][8] outputs of vsd_add_noise_dev and of `prev` / `denoised` of vsd_lcm_step_dev with a noise table and
with none, for two coefficient sets (kept in the file as fp32 hex: the second comes from torch's pow / sqrt).  `dec_in` is tanhf of
`denoised` and would tie the file to a math library: the test checks it across the entry points instead."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import seed_cases as SC  # noqa: E402

OUT = os.path.join(HERE, "scheduler_bits.json")
HW, B = 2 ** 18 + 1, 2
SEED = 0x5C4ED  # of the input hashes
CANARY = 0x7BCD  # fp16 bits of the row after the last image


def half_rows(draw: int, rows: int) -> torch.Tensor:
    """fp16 [rows][8], every value k / 2048 in [-4, 4)"""
    k = (SC.raw_draw(SEED, 0, draw, 2 * rows) >> np.uint32(18)).astype(np.int32) - 8192
    return torch.from_numpy((k.astype(np.float32) / np.float32(2048.0)).astype(np.float16).reshape(rows, 8))


def noise_table(draw: int, hw: int) -> torch.Tensor:
    """fp32 [4][hw], every value k * 2^-21 in [-4, 4)"""
    k = (SC.raw_draw(SEED, 1, draw, hw) >> np.uint32(8)).astype(np.int32) - 2 ** 23
    return torch.from_numpy(np.ascontiguousarray((k.astype(np.float32) * np.float32(2.0 ** -21)).T))


def inputs(hw: int, batch: int = B):
    """(x0, eps, sample, noise) on the host"""
    return half_rows(0, batch * hw), half_rows(1, batch * hw), half_rows(2, batch * hw), noise_table(3, hw)


def coefficient_sets():
    """name -> (add_noise pair, the six of a step) as float32 arrays.  Only the maker calls this: the test reads the recorded hex."""
    from videosd_amd.lcm import LCMSchedule

    six = np.array([0.8321, 0.5547, 0.3071, 0.9517, 0.9123, 0.4095], dtype=np.float32)  # tests/test_seed_gpu.py
    sched = LCMSchedule(0.6, 4)
    return {"seed_test": (six[:2], six),
            "lcm_0.6_4_step_1": (np.array(sched.add_noise_coef(), dtype=np.float32), np.array(sched.step_coef(1), dtype=np.float32))}


def out_rows(ops, rows: int) -> torch.Tensor:
    """fp16 [rows + 1][8] of ones with the canary row at the end: a kernel writes rows [0, rows) alone"""
    t = torch.ones(rows + 1, 8, dtype=torch.float16)
    t[rows] = torch.tensor([CANARY], dtype=torch.int16).view(torch.float16)
    return ops.to_device(t)


def bits(ops, t: torch.Tensor) -> np.ndarray:
    ops.synchronize()
    return t.cpu().numpy().view(np.uint16)


def run_dev(ops, dev_in, pair, six, hw: int, batch: int = B):
    """the product path: one launch per kernel for the whole batch -> name -> uint16 [batch * hw + 1][8] (canary row included)"""
    x0, eps, sample, noise = dev_in
    k2, k6 = ops.to_device(torch.from_numpy(pair.copy())), ops.to_device(torch.from_numpy(six.copy()))
    new = lambda: out_rows(ops, batch * hw)  # noqa: E731
    got = {"add_noise": new(), "prev_noise": new(), "den_noise": new(), "dec_noise": new(), "prev_none": new(), "den_none": new(), "dec_none": new()}
    ops.add_noise_dev(x0, noise, k2, hw, batch, got["add_noise"])
    ops.lcm_step_dev(eps, sample, noise, k6, hw, batch, got["prev_noise"], got["den_noise"], got["dec_noise"])
    ops.lcm_step_dev(eps, sample, None, k6, hw, batch, got["prev_none"], got["den_none"], got["dec_none"])
    return {k: bits(ops, v) for k, v in got.items()}


RECORDED = ("add_noise", "prev_noise", "den_noise", "prev_none", "den_none")


def digest(a: np.ndarray, rows: int) -> str:
    return hashlib.sha256(np.ascontiguousarray(a[:rows]).tobytes()).hexdigest()


def main():
    from videosd_amd import lib as L
    from videosd_amd.ops import HipOps

    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    ops = HipOps(0)
    dev_in = tuple(ops.to_device(t) for t in inputs(HW))
    ver = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.splitlines()
    rec = {"hw": HW, "batch": B, "hipcc": "; ".join(v.strip() for v in ver[:2]), "sets": {}}
    for name, (pair, six) in coefficient_sets().items():
        got = run_dev(ops, dev_in, pair, six, HW)
        rec["sets"][name] = {"add_noise_coef_f32_hex": pair.tobytes().hex(), "step_coef_f32_hex": six.tobytes().hex(),
                             "sha256": {k: digest(got[k], B * HW) for k in RECORDED}}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("library", L.LIB_PATH)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
