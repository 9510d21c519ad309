"""Which kernel and which weight image every eval-path 3-D convolution takes (fused.route / route_phases / PackedW).

The route table tests/golden/conv3d_routes.json was recorded by tools/record_conv3d_routes.py BEFORE the dispatch was rewritten
around route(), when the route was decided once at pack time and once at launch time: the cases of that tool crossed with
every switch setting, with CPU tensors and with GPU tensors (where the fp16 images exist).  The replay must give the same
launch sequences.  The packing tests pin what the rewrite is for: one image per route actually taken, packed at the first
launch that takes it, and no stale image after a switch is flipped."""
import importlib.util
import json
import os

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_conv3d_routes", os.path.join(ROOT, "tools", "record_conv3d_routes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

from occdepth_amd import fused, hip  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "conv3d_routes.json")) as _f:
    GOLDEN = json.load(_f)

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


def _replay(device):
    assert set(GOLDEN[device]) == set(rec.CASES)
    table = rec.record(device)
    bad = []
    for name, rows in table.items():
        labels = GOLDEN["settings_transposed" if rec.CASES[name]["kind"] == "convt2" else "settings"]
        want = GOLDEN[device][name]
        assert len(rows) == len(want) == len(labels), name
        bad += [(name, label, GOLDEN["sequences"][w], got) for label, w, got in zip(labels, want, rows) if GOLDEN["sequences"][w] != got]
    assert not bad, f"{len(bad)} launch sequences differ from the recorded table; the first: {bad[0]}"


def test_route_table_cpu():
    assert GOLDEN["settings"] == [label for label, _ in rec.settings()]
    assert GOLDEN["settings_transposed"] == [label for label, _ in rec.settings(transposed=True)]
    _replay("cpu")


@pytest.mark.gpu
def test_route_table_cuda():
    _replay("cuda")
    used = {GOLDEN["sequences"][i][0].split()[0] + " " + GOLDEN["sequences"][i][0].split()[1]
            for rows in GOLDEN["cuda"].values() for i in rows}
    assert {"conv3d_f16x2 -", "conv3d_bf16 f16x2", "conv3d_phases f16x2"} <= used       # the table does cover the fp16 routes
    for name in ("head_32_32_inf_weight", "small_128_128_inf_weight", "convt_s2_128_64_inf_weight"):   # one Inf: bf16x3
        assert not any("f16x2" in line for i in GOLDEN["cuda"][name] for line in GOLDEN["sequences"][i]), name


DEFAULTS = dict(BF16X3="head", HEAD_SPLIT="f16x2", K2B_SPLIT="f16x2", BF16X3_SMALLVOL=True, BF16X3_DILATED=False,
                PHASES_ONE_LAUNCH=True, PHASES_X3=True, SMALLVOL_KERNELS=((3, 3, 3),))


def _plan(device, cin, cout, dims, k=3):
    torch.manual_seed(1)
    conv = nn.Conv3d(cin, cout, k, padding=k // 2, bias=False).to(device)
    x = hip.Vox(torch.empty((1,) + dims + (cin,), device=device), cin)
    return conv, fused.ConvPlan(conv, nn.BatchNorm3d(cout).to(device).eval()), x


@pytest.mark.parametrize("device", DEVICES)
def test_images_are_packed_per_route_taken(device):
    """A head-geometry plan packs ONE image at its first launch (the fp16 one on the GPU; CPU tensors have no fp16 form and
    take bf16x3), one more when a switch sends it to another route, nothing when the switch goes back, and again one after an
    in-place change of the weight."""
    conv, plan, x = _plan(device, 32, 32, rec.BIG)
    first = "f16x2" if device == "cuda" else "x3"
    second = ["x3"] if device == "cuda" else []
    log, packs = [], []
    with rec.switches(DEFAULTS), rec.stubbed(log, packs), torch.no_grad():
        plan(x)
        assert packs == [first] and log[-1].split()[0] == ("conv3d_f16x2" if device == "cuda" else "conv3d_bf16")
        plan(x)
        assert packs == [first]
        fused.set_head_split("bf16x3")
        plan(x)
        assert packs == [first] + second and log[-1].startswith("conv3d_bf16 split3 x3")
        fused.set_head_split("f16x2")
        plan(x)
        assert packs == [first] + second and log[-1] == log[0]
        fused.set_bf16x3(False)
        plan(x)
        assert packs[-1] == "f32" and log[-1].startswith("conv3d - f32")
        fused.set_bf16x3("head")
        n = len(packs)
        plan(x)
        assert len(packs) == n and log[-1] == log[0]
        conv.weight.mul_(1.0)                                   # same values, new _version: the holder and its images go
        plan(x)
        assert packs[n:] == [first] and log[-1] == log[0]


@pytest.mark.parametrize("device", DEVICES)
def test_switch_flipped_after_first_call_reroutes(device):
    """fused.BF16X3_SMALLVOL and SMALLVOL_KERNELS were in no plan's cache key: a plan prepared under one value kept its image
    set under the other.  Now the next launch takes the route of the new value."""
    _, plan, x = _plan(device, 128, 128, rec.SMALL)
    split = "conv3d_bf16 f16x2 f16x2" if device == "cuda" else "conv3d_bf16 split3 x3"
    log = []
    with rec.switches(DEFAULTS), rec.stubbed(log), torch.no_grad():
        fused.BF16X3_SMALLVOL = False
        plan(x)
        assert log[-1].startswith("conv3d - f32")
        fused.BF16X3_SMALLVOL = True
        plan(x)
        assert log[-1].startswith(split)
        fused.BF16X3_SMALLVOL = False
        plan(x)
        assert log[-1].startswith("conv3d - f32")
        _, k1, _ = _plan(device, 128, 128, rec.SMALL, k=1)
        fused.BF16X3_SMALLVOL = True
        k1(x)
        assert log[-1].startswith("conv3d - f32 k111")
        fused.SMALLVOL_KERNELS = ((3, 3, 3), (1, 1, 1))
        k1(x)
        assert log[-1].startswith("conv3d_bf16 split3 x3 k111")


def test_switch_errors_name_the_variable():
    for setter, env in ((fused.set_wino_split, "OCCDEPTH_WINO_SPLIT"), (fused.set_head_split, "OCCDEPTH_HEAD_SPLIT"),
                        (fused.set_k2b_split, "OCCDEPTH_K2B_SPLIT"), (fused.set_bf16x3, "OCCDEPTH_BF16X3")):
        with pytest.raises(ValueError, match=env + "='fp8': expected "):
            setter("fp8")
    saved = fused.BF16X3
    try:
        fused.set_bf16x3(True)
        assert fused.BF16X3 == "all"
        fused.set_bf16x3("head")
        assert fused.BF16X3 == "head"
        fused.set_bf16x3(0)
        assert fused.BF16X3 is False
    finally:
        fused.set_bf16x3(saved)
