"""The host half of a plan's live options (include/vsd.h vsd_lcm_timesteps, videosd_amd/plan.py format 2), no GPU needed: the C
schedule is lcm.lcm_timesteps in the same double arithmetic, and the format's fixed points."""
import ctypes as C
import json
import os

import pytest

from videosd_amd import lib as L
from videosd_amd.lcm import lcm_timesteps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(L.LIB_PATH):
        from videosd_amd import build

        build.build(verbose=False)
    return L.load()


def _c_timesteps(strength, steps):
    out = (C.c_int * max(steps, 1))()
    n = C.c_int(-1)
    rc = _lib().vsd_lcm_timesteps(strength, steps, out, C.byref(n))
    return rc, [int(out[i]) for i in range(max(n.value, 0))]


def test_the_c_schedule_is_the_python_schedule_for_every_slider_position():
    for k in range(2, 101):
        for steps in (1, 2, 3, 4, 8, 20, 50):
            rc, ts = _c_timesteps(k / 100, steps)
            assert rc == 0 and ts == lcm_timesteps(k / 100, steps), (k, steps, ts)


def test_the_c_schedule_gives_the_recorded_timesteps_of_the_reference():
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "lcm_scheduler.json")))["timesteps"]
    assert len(cases) == 17
    for c in cases:
        rc, ts = _c_timesteps(c["strength"], c["steps"])
        assert rc == 0 and ts == [int(t) for t in c["timesteps"]], c


@pytest.mark.parametrize("strength,origin", [(0.58, 28), (0.29, 14), (0.14, 7), (0.07, 3)])
def test_the_product_is_truncated_as_a_double(strength, origin):
    """50 * 0.58 = 28.999..., 50 * 0.29 = 14.499..., 50 * 0.14 = 7.000...01, 50 * 0.07 = 3.500...04: int() of the DOUBLE product"""
    assert int(50 * strength) == origin
    rc, ts = _c_timesteps(strength, 50)
    assert rc == 0 and len(ts) == origin and ts[0] == 20 * origin - 1 and ts == lcm_timesteps(strength, 50)
    for steps in (1, 2, 4):
        assert _c_timesteps(strength, steps) == (0, lcm_timesteps(strength, steps))


def test_an_empty_schedule_and_bad_arguments_are_errors():
    with pytest.raises(ValueError):
        lcm_timesteps(0.01, 4)
    for strength, steps in ((0.01, 4), (0.0, 1), (-0.5, 2), (float("nan"), 2), (0.5, 0), (0.5, -1)):
        rc, ts = _c_timesteps(strength, steps)
        assert rc == -1 and ts == [], (strength, steps)
    n = C.c_int()
    assert _lib().vsd_lcm_timesteps(0.5, 2, None, C.byref(n)) == -1


def test_the_signature_tags_cover_every_entry_point_and_hash_stably():
    from videosd_amd import plan as P

    tags = P.signature_tags()
    assert [t.split(":")[0] for t in tags] == P.PLAN_FUNCS
    for t in tags:
        name, letters = t.split(":")
        assert len(letters) == len(L.SIGNATURES[name][1]) - 1 and set(letters) <= set("pifdo")
    assert dict(t.split(":") for t in tags)["vsd_conv_gemm_group"] == "dip"
    h = P.signature_hash()
    assert 0 < h < 1 << 64 and h == P.signature_hash()
    committed = open(os.path.join(ROOT, "videosd_amd", "csrc", "plan_dispatch.inc")).read()
    for t in tags:
        assert f'"{t}",' in committed
    assert P.VERSION == 1 and P.FORMAT_VERSION == 2 and P.HEADER_BYTES == 76 and P.OTHER_PROGRAM == 1
    assert "VSD_PLAN_OTHER_PROGRAM = 1" in open(os.path.join(ROOT, "include", "vsd.h")).read()


def test_rows_of_the_coefficient_table_give_the_engines_constant_block():
    """The gather of csrc/plan_options.hip restated on the host over the exporter's table: for every slider position the block is bit
    for bit what Engine._write_constants uploads (the same expressions of lcm.LCMSchedule, the scales as one fp32 multiply)."""
    import numpy as np
    import torch

    from videosd_amd.lcm import LCMSchedule
    from videosd_amd.plan import OPT_ROWS, option_coefficients

    nres = 13
    coef = option_coefficients(nres).numpy()
    assert coef.dtype == np.float32 and coef.shape == (OPT_ROWS * 6 + nres,)
    for k in range(2, 101):
        for steps in (1, 2, 4, 50):
            s = LCMSchedule(k / 100, steps)
            n = len(s)
            scale = 0.05 * k
            vals = list(s.add_noise_coef())
            for i in range(n):
                vals += [float(x) for x in s.step_coef(i)]
            vals += (torch.logspace(-1, 0, nres) * float(scale)).tolist()
            want = torch.tensor(vals, dtype=torch.float32).numpy()
            row = [(t + 1) // 20 - 1 for t in s.timesteps]
            assert all(20 * r + 19 == t and 0 <= r < OPT_ROWS for r, t in zip(row, s.timesteps))
            got = np.zeros(2 + 6 * n + nres, np.float32)
            got[0:2] = coef[row[0] * 6 + 4:row[0] * 6 + 6]
            for i in range(n):
                got[2 + 6 * i:6 + 6 * i] = coef[row[i] * 6:row[i] * 6 + 4]
                nxt = row[min(i + 1, n - 1)]
                got[6 + 6 * i:8 + 6 * i] = coef[nxt * 6:nxt * 6 + 2]
            got[2 + 6 * n:] = coef[OPT_ROWS * 6:] * np.float32(scale)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, steps)
