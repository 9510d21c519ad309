"""Routing of the last on-the-fly-split 2-D GEMMs onto the f16x2 weight image, through the model's own operand builders: one
decoder level (UpSampleBN: the channel-major Winograd-domain path, hip.WinoCM) and one MBConv block (InvertedResidual: the
project convolution with gate and skip on K16's tile variants) at small sizes, under OCCDEPTH_GEMM_SPLIT = f16x2 and = bf16x3.
The host rules (hip.wino_cm_wins, hip.tile_f16x2_wins) are measured on the frame's geometries and turn these small launches
down; the tests open them so that the switch alone decides."""
import copy

import pytest
import torch

DEV = "cuda"
# the bound tests/test_gemm_f16x2.py puts on a decoder level between the two settings of the switch
MODEL_TOL = 1e-5


@pytest.fixture(scope="module")
def hip(hip_lib):
    from occdepth_amd import hip as h
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return h


def _randomise_bn(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.2)


def _families(prof):
    return [k.split(":")[0] for k in prof.rows]


@pytest.mark.gpu
def test_decoder_level_takes_the_channel_major_path_under_f16x2(hip, monkeypatch):
    from occdepth_amd import fused
    from occdepth_amd.models.unet2d import UpSampleBN
    torch.manual_seed(3)
    up = UpSampleBN(skip_input=24 + 16, output_features=24)
    _randomise_bn(up)
    up.eval()
    x, skip = torch.randn(2, 24, 3, 5), torch.randn(2, 16, 6, 9)
    with torch.no_grad():
        ref = copy.deepcopy(up).double()(x.double(), skip.double())
    up = up.to(DEV)
    monkeypatch.setattr(UpSampleBN, "WINOGRAD_MIN_CIN", 8)                 # the second convolution (24 -> 24) on the unfused path
    monkeypatch.setattr(hip, "wino_cm_wins", lambda *a: True)
    saved = fused.GEMM_SPLIT
    try:
        outs = {}
        for mode in ("f16x2", "bf16x3"):
            hip.set_gemm_split(mode)
            with torch.no_grad(), hip.profile() as prof:
                outs[mode] = up(x.to(DEV), skip.to(DEV))
            fam = _families(prof)
            if mode == "f16x2":
                assert "wino_input_cm" in fam and "wino_output_cm" in fam and "wino_input" not in fam, list(prof.rows)
                assert any(k.startswith("gemm_f32x3_preA:24x30x24 b16") and k.endswith(" f16x2") for k in prof.rows), list(prof.rows)
            else:
                assert "wino_input" in fam and "wino_output" in fam and "wino_input_cm" not in fam, list(prof.rows)
                assert any(k.startswith("gemm_f32x3:30x24x24 b16") for k in prof.rows), list(prof.rows)
            err = float((outs[mode].double().cpu() - ref).abs().max() / ref.abs().max())
            print(f"UpSampleBN level, GEMM split {mode}: max rel err vs float64 {err:.2e}")
            assert outs[mode].shape == ref.shape and err < MODEL_TOL, (mode, err)
    finally:
        fused.set_gemm_split(saved)


@pytest.mark.gpu
def test_mbconv_project_takes_the_image_under_f16x2(hip, monkeypatch):
    from occdepth_amd import fused
    from occdepth_amd.models.efficientnet import InvertedResidual
    torch.manual_seed(4)
    block = InvertedResidual(48, 48, 3, 1, 6)                              # expand 48 -> 288, project 288 -> 48 with gate + skip
    _randomise_bn(block)
    block.eval()
    x = torch.randn(2, 48, 40, 40)                                          # 3200 pixels: the project convolution goes to K16
    with torch.no_grad():
        ref = copy.deepcopy(block).double()(x.double())
    block = block.to(DEV)
    monkeypatch.setattr(hip, "tile_f16x2_wins", lambda *a: True)
    saved = fused.GEMM_SPLIT
    try:
        for mode in ("f16x2", "bf16x3"):
            hip.set_gemm_split(mode)
            with torch.no_grad(), hip.profile() as prof:
                out = block(x.to(DEV))
            rows = [k for k in prof.rows if ":48x1600x288 b2" in k]
            assert len(rows) == 1, list(prof.rows)
            if mode == "f16x2":
                assert rows[0].split(":")[0] == "gemm_f32x3_preA" and rows[0].endswith(" f16x2"), rows
            else:
                assert rows[0].split(":")[0] == "gemm_f32x3" and not rows[0].endswith(" f16x2"), rows
            err = float((out.double().cpu() - ref).abs().max() / ref.abs().max())
            print(f"InvertedResidual block, GEMM split {mode}: max rel err vs float64 {err:.2e}")
            assert out.shape == ref.shape and err < MODEL_TOL, (mode, err)
    finally:
        fused.set_gemm_split(saved)
