"""The scheduler kernels' bits on the MI355X (include/vsd.h THE SCHEDULER ARITHMETIC; csrc/noise.hip): the digests that
tests/golden/make_scheduler_bits.py recorded from the commit before the six entry points shared one body, and the entry points against each
other -- vsd_add_noise / vsd_lcm_step (coefficients by value, image by image) give the rows of the `_dev` forms bit for bit.  (The seeded
forms against fill + `_dev`: tests/test_seed_gpu.py.)

Shapes: hw = 2^18 + 1, B = 2 for the digests (the maker's docstring says why so large: a wrong contraction flips tens of fp16 results per
million); hw in {1, 255, 257} for the edges: a lone thread, one short of and one past a workgroup."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_scheduler_bits as M  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ["lcm_0.6_4_step_1", "seed_test"]


def _golden():
    g = json.load(open(M.OUT))
    assert (g["hw"], g["batch"]) == (M.HW, M.B) and sorted(g["sets"]) == NAMES
    return g


def _coef(name):
    """(add_noise pair, the six of a step) as recorded: float32 arrays"""
    s = _golden()["sets"][name]
    return tuple(np.frombuffer(bytes.fromhex(s[k]), dtype=np.float32) for k in ("add_noise_coef_f32_hex", "step_coef_f32_hex"))


@pytest.fixture(scope="module")
def ops():
    from videosd_amd.ops import HipOps

    return HipOps(0)


@pytest.fixture(scope="module")
def big(ops):
    """the maker's inputs on the device, and per coefficient set the outputs of the `_dev` forms (computed once, left unchanged)"""
    dev_in = tuple(ops.to_device(t) for t in M.inputs(M.HW))
    return dev_in, {name: M.run_dev(ops, dev_in, *_coef(name), M.HW) for name in NAMES}


def _host_forms(ops, dev_in, pair, six, hw, batch):
    """vsd_add_noise / vsd_lcm_step image by image, with `dec_in` and (the `_nodec` entries) without -> the names of M.run_dev"""
    x0, eps, sample, noise = dev_in
    rows = lambda t, b: t[b * hw:(b + 1) * hw]  # noqa: E731
    new = lambda: M.out_rows(ops, batch * hw)  # noqa: E731
    names = ("add_noise", "prev_noise", "den_noise", "dec_noise", "prev_none", "den_none", "dec_none", "prev_noise_nodec", "den_noise_nodec",
             "prev_none_nodec", "den_none_nodec")
    got = {k: new() for k in names}
    for b in range(batch):
        ops.add_noise(rows(x0, b), noise, float(pair[0]), float(pair[1]), hw, rows(got["add_noise"], b))
        for tag, nz in (("noise", noise), ("none", None)):
            ops.lcm_step(rows(eps, b), rows(sample, b), nz, six, hw, rows(got["prev_" + tag], b), rows(got["den_" + tag], b), rows(got["dec_" + tag], b))
            ops.lcm_step(rows(eps, b), rows(sample, b), nz, six, hw, rows(got["prev_" + tag + "_nodec"], b), rows(got["den_" + tag + "_nodec"], b), None)
    return {k: M.bits(ops, v) for k, v in got.items()}


def _assert_forms_equal(host, dev, where):
    for k, a in host.items():
        assert np.array_equal(a, dev[k.replace("_nodec", "")]), (where, k)  # (the canary row included)


@pytest.mark.parametrize("name", NAMES)
def test_the_dev_kernels_give_the_recorded_bits(big, name):
    _, dev = big
    golden = _golden()
    for k in M.RECORDED:
        d = M.digest(dev[name][k], M.B * M.HW)
        print(name, k, d)
    for k in M.RECORDED:
        assert M.digest(dev[name][k], M.B * M.HW) == golden["sets"][name]["sha256"][k], (name, k, "recorded under " + golden["hipcc"])
    assert np.array_equal(dev[name]["prev_none"], dev[name]["den_none"])  # no noise: prev = denoised


@pytest.mark.parametrize("name", NAMES)
def test_the_host_coefficient_forms_give_the_dev_rows_bit_for_bit(ops, big, name):
    dev_in, dev = big
    _assert_forms_equal(_host_forms(ops, dev_in, *_coef(name), M.HW, M.B), dev[name], name)


@pytest.mark.parametrize("hw", [1, 255, 257])
def test_the_edges_of_the_grid(ops, hw):
    pair, six = _coef("lcm_0.6_4_step_1")
    dev_in = tuple(ops.to_device(t) for t in M.inputs(hw))
    dev = M.run_dev(ops, dev_in, pair, six, hw)
    _assert_forms_equal(_host_forms(ops, dev_in, pair, six, hw, M.B), dev, hw)
    for k, a in dev.items():
        assert (a[:M.B * hw, 4:] == 0).all(), (hw, k)  # channels 4..7 are written, as zero (the buffers held ones)
        assert a[:M.B * hw, :4].any() and (a[M.B * hw] == M.CANARY).all(), (hw, k)  # the row after the last image is untouched
    # every output of a step is optional
    x0, eps, sample, noise = dev_in
    k6 = ops.to_device(torch.from_numpy(six.copy()))
    for keep in range(3):
        outs = [M.out_rows(ops, M.B * hw) if j == keep else None for j in range(3)]
        ops.lcm_step_dev(eps, sample, noise, k6, hw, M.B, *outs)
        assert np.array_equal(M.bits(ops, outs[keep]), dev[("prev_noise", "den_noise", "dec_noise")[keep]]), (hw, keep)
        outs = [M.out_rows(ops, hw) if j == keep else None for j in range(3)]
        ops.lcm_step(eps[:hw], sample[:hw], None, six, hw, *outs)
        assert np.array_equal(M.bits(ops, outs[keep])[:hw], dev[("prev_none", "den_none", "dec_none")[keep]][:hw]), (hw, keep)
    ops.lcm_step_dev(eps, sample, noise, k6, hw, M.B, None, None, None)
    ops.synchronize()
