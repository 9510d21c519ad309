"""Which entry point, operand forms and kernel every eval-path 2-D GEMM takes (hip.gemm_route / hip.GemmWeights, and the
library's occd_gemm_f32x3_route).

tests/golden/gemm_routes.json was recorded by tools/record_gemm_routes.py BEFORE the dispatch was rewritten around
gemm_route(), when the kernel was chosen at pack time (matmul_operand), again at launch time (matmul's image logic and a
host-side mirror of the library's panel rule) and a third time in the library: the cases of that tool crossed with its
switch settings, with CPU tensors and with GPU tensors, and every distinct hint-0 geometry launched once under a kernel
trace.  The replay must give the same launch sequences; the library's route query must name the kernels the trace shows.
The packing tests pin what the rewrite is for: one image per route actually taken, packed at the first launch that takes
it, none held for a route no launch takes.  The numerical tests hold hip.matmul on GemmWeights bit-equal to the explicit
launch on a hand-built image."""
import collections
import importlib.util
import json
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_gemm_routes", os.path.join(ROOT, "tools", "record_gemm_routes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

from occdepth_amd import fused, hip  # noqa: E402
from occdepth_amd.models import efficientnet as en  # noqa: E402
from occdepth_amd.models import unet2d  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "gemm_routes.json")) as _f:
    GOLDEN = json.load(_f)
SEQ = GOLDEN["sequences"]
DEV = "cuda"


def _replay(device):
    assert GOLDEN["settings"] == [label for label, _ in rec.settings()]
    assert set(GOLDEN[device]) == set(rec.CASES)                               # no case skipped, none added unrecorded
    table = rec.record(device)
    bad, more = [], []
    for name, rows in table.items():
        want = GOLDEN[device][name]
        assert len(rows) == len(want) == len(GOLDEN["settings"]), name
        for label, (w_log, w_packs), (log, packs) in zip(GOLDEN["settings"], want, rows):
            if SEQ[w_log] != log:
                bad.append((name, label, SEQ[w_log], log))
            if collections.Counter(packs) - collections.Counter(SEQ[w_packs]):
                more.append((name, label, SEQ[w_packs], packs))
    assert not bad, f"{len(bad)} launch sequences differ from the recorded table; the first: {bad[0]}"
    assert not more, f"{len(more)} settings pack an image the old dispatch did not; the first: {more[0]}"
    return table


def test_route_table_cpu():
    _replay("cpu")


@pytest.mark.gpu
def test_route_table_cuda():
    table = _replay("cuda")
    lines = {line for rows in GOLDEN["cuda"].values() for log, _ in rows for line in SEQ[log]}
    forms = {" ".join(line.split()[:3]) for line in lines}
    assert {"gemm_x3 A=f16x2 B=f32", "gemm_x3 A=bf16x3 B=f32", "gemm_x3 A=f32 B=bf16x3", "gemm_x3 A=f32 B=f32",
            "gemm_x3_splitk A=f16x2 B=f32", "gemm_x3_splitk A=bf16x3 B=f32", "conv1x1 k11 shift", "torch.matmul A=f32 B=f32"} <= forms
    for name in ("matmul_inf_weight", "project_inf_weight", "project_k16_inf_weight", "expand_inf_weight", "expand_small_inf_weight",
                 "tap_inf_weight", "head_inf_weight", "wino_1280_1280_inf_weight"):                   # one Inf: never f16x2
        assert not any("f16x2" in line for log, _ in GOLDEN["cuda"][name] for line in SEQ[log]), name
    # what the rewrite is for: the tap matrices no longer pack K11's form beside their image, no setting packs two images
    default = GOLDEN["settings"].index("default")
    for name, rows in table.items():
        if rec.CASES[name]["kind"] == "tap":
            assert not any(p.startswith("k11") for p in rows[default][1]), (name, rows[default][1])
            assert len(rows[default][1]) == len(rows[default][0]) == 1


# the tile variants of csrc/gemm_x3.hip (kVariantsG) by their template arguments MT, NT, WM, WN
VARIANTS = {(2, 2, 4, 2): 0, (2, 2, 2, 2): 1, (2, 1, 2, 2): 2, (1, 1, 2, 2): 3, (2, 2, 1, 4): 4}


def test_library_route_names_the_recorded_kernels():
    """occd_gemm_f32x3_route (host code) against the kernel trace of every hint-0 geometry of the table, recorded at the parent:
    kernel family and variant from the traced kernel's name, the grid and workgroup size from the variant's tile."""
    kernels = GOLDEN["kernels"]
    assert len(kernels) >= 80 and {"gemm_x3_kernel", "gemm_x3_panel_kernel", "gemm_x3_ws_kernel"} == {k["kernel"].split("<")[0] for k in kernels}
    seen = set()
    for k in kernels:
        M, N, K, batch = k["M"], k["N"], k["K"], k["batch"]
        t = tuple(int(v) for v in re.findall(r"\d+", k["kernel"].split("<")[1]))
        got = hip.gemm_x3_route(M, N, K, batch, k["pre"], bool(k["plain"]))
        if "panel" in k["kernel"]:
            want, wg = ("panel", t[1]), 512
            assert k["grid"][0] % -(-N // (32 * t[1])) == 0                               # row ranges x column panels
            assert (t[3] if len(t) > 3 else 3) == (2 if k["pre"] == hip.GEMM_PRE_F16X2 else 3)
        elif "ws" in k["kernel"]:
            want, wg = ("ws", 0), 512
            assert k["grid"][0] == -(-M // 256) * -(-N // 128)
        else:
            MT, NT, WM, WN, ks = t[0], t[1], t[2], t[3], t[6]
            want, wg = ("ksplit" if ks == 4 else "tile", VARIANTS[t[:4]]), WM * WN * 64 * ks
            assert k["grid"][0] == -(-M // (MT * WM * 32)) * -(-N // (NT * WN * 32))
        assert got == want and k["wg"] == wg and k["grid"][1] == batch, (k, got)
        seen.add(want)
    assert {("panel", 1), ("panel", 2), ("ws", 0), ("ksplit", 3), ("tile", 0), ("tile", 3)} <= seen
    assert hip.gemm_x3_route(256, 100, 64, 2, 0, True, tile_hint=8) is None               # what the launch refuses, the query refuses
    assert hip.gemm_x3_route(256, 100, 60, 2) is None and hip.gemm_x3_route(256, 3, 64, 2) is None
    assert hip.gemm_x3_route(256, 100, 64, 2, 1, True, tile_hint=8) == ("panel", 2)


DEFAULTS = rec.DEFAULTS


@pytest.mark.gpu
def test_images_are_packed_per_route_taken():
    """A tap matrix packs ONE image at its first launch, one more when set_gemm_split or GEMM_X3_PANEL sends the launch
    elsewhere, nothing on the way back, again one after an in-place change of the weight -- and K11's form only when a launch
    routes to K11."""
    torch.manual_seed(1)
    up = unet2d.UpSampleBN(skip_input=160 + 8, output_features=80).to(DEV).eval()
    x, skip = torch.empty(2, 160, 20, 30, device=DEV), torch.empty(2, 8, 40, 60, device=DEV)
    call = lambda: up._first_conv_upconv(x, skip, up._net[0], up._net[1], up._net[2])
    log, packs = [], []
    with rec.switches(DEFAULTS), rec.stubbed(log, packs), torch.no_grad():
        call()
        assert packs == ["f16x2-a 720x160"] and log[-1].startswith("gemm_x3 A=f16x2")
        call()
        assert len(packs) == 1
        hip.set_gemm_split("bf16x3")
        call()
        assert packs[1:] == ["bf16x3-a 720x160"] and log[-1].startswith("gemm_x3 A=bf16x3")
        hip.set_gemm_split("f16x2")
        call()
        assert len(packs) == 2 and log[-1] == log[0]
        hip.GEMM_X3_PANEL = False
        call()
        assert len(packs) == 2 and log[-1].startswith("gemm_x3 A=f32")
        hip.GEMM_X3_PANEL = True
        call()
        assert len(packs) == 2 and log[-1] == log[0]
        up._net[0].weight.mul_(1.0)                                   # same values, new _version: the holder and its images go
        call()
        assert packs[2:] == ["f16x2-a 720x160"] and log[-1] == log[0]
        unet2d.UpSampleBN.UPCONV_LIB_BELOW = 0
        try:
            call()
        finally:
            unet2d.UpSampleBN.UPCONV_LIB_BELOW = 1 << 62
        assert packs[3:] == ["k11 720x160"] and log[-1].startswith("conv1x1 k11")


@pytest.mark.gpu
def test_project_on_k21_holds_one_image():
    torch.manual_seed(2)
    owner, conv, bn = torch.nn.Module(), torch.nn.Conv2d(960, 160, 1, bias=False).to(DEV).eval(), torch.nn.BatchNorm2d(160).to(DEV).eval()
    y, gate, skip = torch.empty(2, 960, 24, 77, device=DEV), torch.empty(2, 960, device=DEV), torch.empty(2, 160, 24, 77, device=DEV)
    log, packs = [], []
    with rec.switches(DEFAULTS), rec.stubbed(log, packs), torch.no_grad():
        en.project_conv(owner, conv, bn, y, gate, skip)
        en.project_conv(owner, conv, bn, y, gate, skip)
    assert packs == ["f16x2-a 160x960"] and log[0].startswith("gemm_x3_splitk A=f16x2") and log[0] == log[1]
    (key, w, shift), = owner._gemm_cache.values()
    assert list(w.images) == ["f16x2"] and set(owner.__dict__) >= {"_gemm_cache"} and "_splitk_cache" not in owner.__dict__ \
        and "_pw_cache" not in owner.__dict__


@pytest.fixture
def split(request):
    saved = fused.GEMM_SPLIT
    hip.set_gemm_split(request.param)
    yield request.param
    fused.set_gemm_split(saved)


both_splits = pytest.mark.parametrize("split", ["f16x2", "bf16x3"], indirect=True)


def _operands(M, N, K, batch, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.randn(M, K, generator=g) / K ** 0.5).to(DEV), torch.randn(batch, K, N, generator=g).to(DEV),
            torch.randn(M, generator=g).to(DEV))


@pytest.mark.gpu
@both_splits
def test_matmul_panel_equals_the_explicit_launch(hip_lib, split):
    a, b, bias = _operands(256, 70, 64, 2, 1)
    w = hip.GemmWeights(a, "a", split="switch")
    with hip.profile() as prof:
        got = hip.matmul(w, b, bias=bias, act="swish")
    assert [k.split(":")[0] for k in prof.rows if "pack" not in k] == ["gemm_f32x3_panel"] and list(w.images) == [split]
    assert torch.equal(got, hip.gemm_x3(hip.GemmPacked(a, "a", split=split), b, bias=bias, act="swish"))


@pytest.mark.gpu
@both_splits
def test_matmul_tile_image_with_res_and_k_scale_equals_the_explicit_launch(hip_lib, split):
    a, b, bias = _operands(48, 1500, 64, 2, 2)
    res, ks = torch.randn(2, 48, 1500, device=DEV), torch.rand(2, 64, device=DEV)
    w = hip.GemmWeights(a, "a", split="switch", small=True)
    assert hip.tile_f16x2_wins(48, 1500, 64, 2)
    got = hip.matmul(w, b, bias=bias, res=res, k_scale=ks)
    xa = hip.GemmPacked(a, "a", split="f16x2") if split == "f16x2" else a       # (bf16x3: float32 operands, split on the fly)
    assert list(w.images) == (["f16x2"] if split == "f16x2" else [])
    assert torch.equal(got, hip.gemm_x3(xa, b, bias=bias, res=res, k_scale=ks))


@pytest.mark.gpu
@both_splits
def test_matmul_presplit_equals_the_explicit_launch(hip_lib, split, monkeypatch):
    a, b, bias = _operands(256, 70, 856, 2, 3)                                  # K = 856: beyond the panel kernel
    w = hip.GemmWeights(a, "a", split="switch")
    assert hip.gemm_route(256, 70, 856, 2, a=w).a == "f32"
    monkeypatch.setattr(hip, "presplit_wins", lambda *g: True)                  # (the rule admits chip-filling launches only)
    with hip.profile() as prof:
        got = hip.matmul(w, b, bias=bias)
    assert [k.split(":")[0] for k in prof.rows if "pack" not in k] == ["gemm_f32x3_preA"] and list(w.images) == [split]
    assert torch.equal(got, hip.gemm_x3(hip.GemmPacked(a, "a", split=split), b, bias=bias))


@pytest.mark.gpu
@both_splits
def test_project_k21_equals_the_explicit_launch(hip_lib, split, monkeypatch):
    torch.manual_seed(4)
    owner, conv, bn = torch.nn.Module(), torch.nn.Conv2d(256, 64, 1, bias=False).to(DEV).eval(), torch.nn.BatchNorm2d(64).to(DEV).eval()
    bn.running_var.uniform_(0.5, 1.5)
    y, gate, skip = torch.randn(2, 256, 5, 8, device=DEV), torch.rand(2, 256, device=DEV), torch.randn(2, 64, 5, 8, device=DEV)
    monkeypatch.setattr(en, "PW_PROJECT_SPLITK_MIN_K", 256)
    monkeypatch.setattr(hip, "splitk_f16x2_wins", lambda *g: True)
    with torch.no_grad(), hip.profile() as prof:
        got = en.project_conv(owner, conv, bn, y, gate, skip)
    assert "gemm_f32x3_splitk" in [k.split(":")[0] for k in prof.rows] and not any(k.startswith("pw_conv") for k in prof.rows), list(prof.rows)
    scale, shift = en.bn_affine_cached(bn)
    wf = (conv.weight.detach().float().flatten(1) * scale.view(-1, 1)).contiguous()
    want = hip.gemm_x3_splitk(hip.GemmPacked(wf, "a", split=split), y.view(2, 256, 40), bias=shift.contiguous(), k_scale=gate,
                              res=skip.view(2, 64, 40))
    assert torch.equal(got, want.view(2, 64, 5, 8))


@pytest.mark.gpu
def test_inf_weight_takes_bf16x3(hip_lib):
    a, b, bias = _operands(256, 70, 64, 2, 5)
    a[3, 5] = float("inf")
    saved = fused.GEMM_SPLIT
    try:
        hip.set_gemm_split("f16x2")
        w = hip.GemmWeights(a, "a", split="switch")
        got = hip.matmul(w, b, bias=bias)
        assert w.images["f16x2"] is None and w.images["bf16x3"].split == "bf16x3"
        want = hip.gemm_x3(hip.GemmPacked(a, "a"), b, bias=bias)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))          # (bit patterns: row 3 is Inf / NaN)
    finally:
        fused.set_gemm_split(saved)
