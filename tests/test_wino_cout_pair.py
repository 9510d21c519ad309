"""K10h's cout-pair form (csrc/wino_conv2d.hip, occd_wino_conv3x3_f16x2_fwd_form with cout_blocks = 2) against today's form of
the same launch (cout_blocks = 1, max_workgroups = -1).

The pair form changes no arithmetic: per accumulator the same MFMAs in the same order, per output the same additions in the
same order, so every comparison is torch.equal on the same packed operand.  Shapes (Cin -> Cout @ B x H x W), the smallest that
reach each way the kernel can go wrong:
  24 -> 40  @2x5x9     two cout blocks, the Cout tail inside the second; Cin no multiple of 16; odd W and H; one partial item
  40 -> 72  @1x6x131   three cout blocks: the last item has no second block; odd W; several tile blocks along x
  16 -> 32  @1x8x64    one cout block: every item is without a second block
   8 -> 24  @2x4x6     ... and Cin below one chunk
  80 -> 160 @1x20x70   five cout blocks; even W; both tilings by tile_hint; several tile blocks along y, a ragged last one
 264 -> 264 @2x4x6     17 chunks, nine cout blocks, few tiles
The pair form has one workgroup per item only: a persistent grid is refused (test_pair_form_has_no_persistent_grid).
"""
import ctypes
import functools

import pytest
import torch

from test_wino_f16x2 import OVERFLOW_AT, check_gates, errors, make, reference

# (B, Cin, Cout, H, W, act, residual, res_first, tile_hint)
SHAPES = [
    (2, 24, 40, 5, 9, "leaky", True, True, 0),
    (1, 40, 72, 6, 131, "relu", True, False, 0),
    (1, 16, 32, 8, 64, "leaky", False, False, 0),
    (2, 8, 24, 4, 6, None, True, True, 0),
    (1, 80, 160, 20, 70, "leaky", True, True, 16),
    (1, 80, 160, 20, 70, "leaky", True, True, 32),
    (2, 264, 264, 4, 6, "swish", False, False, 0),
]
# with and without a residual, before and after every activation, on an odd-width and an even-width shape
VARIANTS = [(B, cin, cout, H, W, act, with_res, res_first, hint)
            for (B, cin, cout, H, W, hint) in ((2, 24, 40, 5, 9, 0), (1, 80, 160, 20, 70, 0))
            for act in (None, "relu", "swish", "leaky")
            for with_res, res_first in ((False, False), (True, True), (True, False))]
VARIANTS = [c for c in VARIANTS if c not in SHAPES]
GATE_CASE = (1, 40, 72, 6, 131, "relu", True, False, 0)
# (cin, cout, H, W) at batch 2: the fused-Winograd launch geometries of the config-2 frame and what the committed rule says
FRAME_GEOMETRIES = {(80, 80, 370, 1220): False, (160, 160, 185, 610): True, (320, 320, 93, 305): True,
                    (128, 128, 47, 153): True, (32, 160, 185, 610): True, (48, 320, 93, 305): True,
                    (224, 1280, 24, 77): True, (80, 640, 47, 153): True, (64, 128, 47, 153): True}


@functools.lru_cache(maxsize=None)
def operands(case):
    from occdepth_amd import hip
    x, w, scale, shift, res = (v.cuda() if v is not None else None for v in make(case))
    return x, hip.wino_pack_weights_f16x2(w, scale), shift, res


def run(case, cout_blocks, x=None, shift=True, out=None, max_workgroups=-1):
    from occdepth_amd import hip
    x0, upk, sh, res = operands(case)
    return hip.conv2d_3x3_fused(x0 if x is None else x, upk, case[2], sh if shift else None, case[5], 0.01, res, res_first=case[7],
                                tile_hint=case[8], out=out, max_workgroups=max_workgroups, cout_blocks=cout_blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPES + VARIANTS)
def test_pair_form_equals_one_block_form_gpu(case, hip_lib):
    want, got = run(case, 1), run(case, 2)
    assert torch.equal(got, want), (case, float((got - want).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[4]])
def test_pair_form_without_shift_gpu(case, hip_lib):
    assert torch.equal(run(case, 2, shift=False), run(case, 1, shift=False)), case


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHAPES)
def test_every_output_is_written_and_nothing_else_gpu(case, hip_lib):
    """y pre-filled with NaN inside a NaN guard band: no NaN is left in y, the band is untouched (a missing second block
    writes nothing)."""
    B, cout, H, W = case[0], case[2], case[3], case[4]
    n, guard = B * cout * H * W, 4096
    buf = torch.full((n + 2 * guard,), float("nan"), device="cuda")
    y = buf[guard:guard + n].view(B, cout, H, W)
    run(case, 2, out=y)
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all()), case
    assert torch.equal(y, run(case, 1)), case


@pytest.mark.gpu
def test_non_finite_behaviour_is_the_same_gpu(hip_lib):
    """Activations at the fp16 staging threshold (|x| >= 8190), an Inf and a NaN: the same bits, non-finite ones included."""
    case = SHAPES[0]
    x = operands(case)[0].clone()
    x[0, 3, 2:4, 4:6] = OVERFLOW_AT
    x[1, 5, 1, 7] = -(OVERFLOW_AT + 100.0)
    x[1, 20, 4, 0] = float("inf")
    x[0, 17, 0, 8] = float("nan")
    want, got = run(case, 1, x=x), run(case, 2, x=x)
    assert not bool(torch.isfinite(want).all()) and bool(torch.isfinite(want).any())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
def test_pair_form_meets_the_float64_gates_gpu(hip_lib):
    """The two gates of test_wino_f16x2 against ATen float64 (max error < 2e-5 of the output maximum, rms <= 2 x K10's): a
    guard against both forms being wrong together."""
    from occdepth_amd import hip
    case = GATE_CASE
    t = make(case)
    x, w, scale, shift, res = (v.cuda() for v in t)
    y_f32 = hip.conv2d_3x3_fused(x, hip.wino_pack_weights(w, scale), case[2], shift, case[5], 0.01, res, res_first=case[7])
    ref = reference(case, *t)
    check_gates(case, errors(run(case, 2), ref), errors(y_f32, ref))


@pytest.mark.gpu
def test_pair_form_has_no_persistent_grid_gpu(hip_lib):
    case = SHAPES[1]
    for grid in (0, 1, 3, 8):
        with pytest.raises(RuntimeError, match="occd_wino_conv3x3_f16x2_fwd_form"):
            run(case, 2, max_workgroups=grid)
    # one cout block per item keeps every grid
    assert torch.equal(run(case, 1, max_workgroups=3), run(case, 1))


def test_entry_point_refuses_other_forms(hip_lib):
    """Host-side: cout_blocks outside {1, 2} is refused before anything else is looked at, and so is a persistent grid of the
    pair form."""
    from occdepth_amd import hip
    a = hip.WinoArgs()
    buf = (ctypes.c_float * 4)()
    a.x = a.upk = a.y = ctypes.cast(buf, ctypes.c_void_p)
    a.batch, a.cin, a.cout, a.H, a.W = 1, 8, 8, 4, 4
    for blocks in (0, 3, 4, -1, 64):
        for grid in (-1, 0, 3):
            assert hip_lib.occd_wino_conv3x3_f16x2_fwd_form(ctypes.byref(a), grid, blocks, None) == -1
    for grid in (0, 1, 256, -2):
        assert hip_lib.occd_wino_conv3x3_f16x2_fwd_form(ctypes.byref(a), grid, 2, None) == -1
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd_form(None, -1, 2, None) == -1
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd_form(ctypes.byref(a), -2, 1, None) == -1
    a.act = 7
    for blocks in (1, 2):
        assert hip_lib.occd_wino_conv3x3_f16x2_fwd_form(ctypes.byref(a), -1, blocks, None) == -1


def test_cout_pair_switch_parses():
    from occdepth_amd import hip
    assert hip._parse_wino_cout_pair("auto") is None
    assert hip._parse_wino_cout_pair("1") is True and hip._parse_wino_cout_pair("0") is False
    for bad in ("", "2", "yes", "-1", "01", "AUTO", "true"):
        with pytest.raises(ValueError):
            hip._parse_wino_cout_pair(bad)
    assert hip.WINO_COUT_PAIR in (None, True, False)


def test_rule_follows_the_committed_table():
    """The nine launch geometries of the frame: the pair form only where profiles/wino_cout_pair_ab.txt has its worst round
    below the one-block form's best; anything unmeasured stays on the one-block form."""
    from occdepth_amd import hip
    for (cin, cout, H, W), want in FRAME_GEOMETRIES.items():
        assert hip.wino_cout_pair_wins(2, cin, cout, H, W) is want, (cin, cout, H, W)
    assert {g for g, w in FRAME_GEOMETRIES.items() if w} == set(hip.WINO_COUT_PAIR_TABLE)
    assert hip.wino_cout_pair_wins(1, 160, 160, 185, 610) is False
    assert hip.wino_cout_pair_wins(2, 160, 160, 185, 611) is False


def test_cout_blocks_needs_the_split_operand():
    """A K10 (float32) operand has no work item to choose: the argument is refused, not ignored."""
    from occdepth_amd import hip
    x, upk = torch.zeros(1, 8, 4, 4), torch.zeros(1)
    with pytest.raises(RuntimeError, match="cout_blocks"):
        hip.conv2d_3x3_fused(x, upk, 8, cout_blocks=2)
