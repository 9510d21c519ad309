"""K10h with persistent workgroups (csrc/wino_conv2d.hip, occd_wino_conv3x3_f16x2_fwd_ex) against the one-item-per-workgroup form.

The persistent form changes no arithmetic: the same float operations per output in the same order, so every comparison with
the form `max_workgroups = -1` is torch.equal on the same packed operand.  Shapes: CASES of test_wino_f16x2 (1, 2, 3, 4 and 11
chunks of 16 input channels -- both patch-buffer parities at the hand-over --, both tilings, odd and even widths, ragged
channels, residual before and after the activation, batch 2), plus two with an even width and a residual; tens of items each.
  max_workgroups = 1: one workgroup walks every item (cout blocks, tile rows, both images: the descriptor base changes mid-walk)
                   3: not a multiple of 8, ragged last round
                   8: one workgroup per XCD
                   0: the automatic grid.  A launch with no more items than the grid has workgroups keeps the one-item form
                      by the host rule, so on these shapes 0 only checks that rule; the persistent body under the automatic grid
                      (a multiple of 8, several rounds, a ragged last one) is what `many_items_cases` is for.
The float64 gates, the poison test and determinism run with a forced persistent grid of 3.
"""
import ctypes

import pytest
import torch

from test_wino_f16x2 import CASES, check_gates, errors, make, reference

# even width WITH a residual (CASES has the two apart): the epilogue reads the residual two pixels at a time there
EVEN_WIDTH_RESIDUAL = [(2, 9, 16, 13, 18, "leaky", True, True, 0), (2, 64, 64, 24, 78, "relu", True, False, 32)]
CASES = list(CASES) + EVEN_WIDTH_RESIDUAL
GRIDS = (1, 3, 8, 0)
GRAPH_CASE = (2, 64, 64, 24, 77, "relu", True, True, 16)
assert GRAPH_CASE in CASES


def many_items_cases():
    """Launches with more items than the device has CUs, so that the automatic grid really is persistent (a multiple of 8,
    a ragged second round).  8 -> 32 n couts on a batch of 2, n cout blocks chosen from the CU count (256 CUs: 7, 280 items):
      64 x 130, 2 x 16 tiling: 40 tile blocks, even width, residual before the activation;
      33 x 129, hint 32 (1 x 32 tiling): 2 x 5 x 3 = 30 tile blocks (256 CUs: n = 9, 270 items), odd width and height,
      residual after the activation."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n16, n32 = cus // 40 + 1, cus // 30 + 1
    assert 40 * n16 > cus and 30 * n32 > cus
    return [(2, 8, 32 * n16, 64, 130, "leaky", True, True, 0), (2, 8, 32 * n32, 33, 129, "relu", True, False, 32)]


def operands(case):
    from occdepth_amd import hip
    x, w, scale, shift, res = (v.cuda() if v is not None else None for v in make(case))
    return x, hip.wino_pack_weights_f16x2(w, scale), shift, res


def run(case, ops, max_workgroups, out=None):
    from occdepth_amd import hip
    x, upk, shift, res = ops
    return hip.conv2d_3x3_fused(x, upk, case[2], shift, case[5], 0.01, res, res_first=case[7], tile_hint=case[8], out=out,
                                max_workgroups=max_workgroups)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_persistent_equals_one_item_per_workgroup_gpu(case, hip_lib):
    ops = operands(case)
    want = run(case, ops, -1)
    for grid in GRIDS:
        got = run(case, ops, grid)
        assert torch.equal(got, want), (case, grid, float((got - want).abs().max()))


@pytest.mark.gpu
def test_automatic_grid_with_more_items_than_cus_gpu(hip_lib):
    """The automatic persistent grid: bit equality with the one-item form, every output written inside a NaN guard band,
    and the float64 gates."""
    from occdepth_amd import hip
    for case in many_items_cases():
        t = make(case)
        ops = operands(case)
        want = run(case, ops, -1)
        for grid in (0, 8, 3):
            assert torch.equal(run(case, ops, grid), want), (case, grid)
        B, cout, H, W = case[0], case[2], case[3], case[4]
        n, guard = B * cout * H * W, 4096
        buf = torch.full((n + 2 * guard,), float("nan"), device="cuda")
        y = buf[guard:guard + n].view(B, cout, H, W)
        run(case, ops, 0, out=y)
        assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all()), case
        assert torch.equal(y, want), case
        x, w, scale, shift, res = (v.cuda() for v in t)
        y_f32 = hip.conv2d_3x3_fused(x, hip.wino_pack_weights(w, scale), cout, shift, case[5], 0.01, res, res_first=case[7],
                                     tile_hint=case[8])
        check_gates(case, errors(y, ref := reference(case, *t)), errors(y_f32, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_every_output_is_written_and_nothing_else_gpu(case, hip_lib):
    """y pre-filled with NaN inside a NaN guard band: no NaN is left in y, the band is untouched."""
    ops = operands(case)
    B, cout, H, W = case[0], case[2], case[3], case[4]
    n, guard = B * cout * H * W, 4096
    want = run(case, ops, -1)
    for grid in (-1, 3, 8):
        buf = torch.full((n + 2 * guard,), float("nan"), device="cuda")
        y = buf[guard:guard + n].view(B, cout, H, W)
        run(case, ops, grid, out=y)
        assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all()), (case, grid)
        assert torch.equal(y, want), (case, grid)


@pytest.mark.gpu
def test_deterministic_and_graph_replay_gpu(hip_lib):
    case = GRAPH_CASE
    ops = operands(case)
    eager = run(case, ops, 3)
    assert torch.equal(eager, run(case, ops, 3))
    assert torch.equal(run(case, ops, 8), run(case, ops, 8))
    y = torch.empty_like(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(case, ops, 3, out=y)
    for _ in range(3):
        y.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_persistent_meets_the_float64_gates_gpu(case, hip_lib):
    """The two gates of test_wino_f16x2 against ATen float64: max error < 2e-5 of the output maximum, rms <= 2 x K10's; the
    persistent kernel forced by a grid of 3 (the automatic grid would keep the one-item form on these shapes)."""
    from occdepth_amd import hip
    t = make(case)
    ref = reference(case, *t)
    ops = operands(case)
    x, w, scale, shift, res = (v.cuda() if v is not None else None for v in t)
    y_f32 = hip.conv2d_3x3_fused(x, hip.wino_pack_weights(w, scale), case[2], shift, case[5], 0.01, res, res_first=case[7],
                                 tile_hint=case[8])
    check_gates(case, errors(run(case, ops, 3), ref), errors(y_f32, ref))


def test_max_workgroups_validation(hip_lib):
    """Host-side: a grid below -1 is refused before anything else is looked at; the other checks are K10h's."""
    from occdepth_amd import hip
    a = hip.WinoArgs()
    buf = (ctypes.c_float * 4)()
    a.x = a.upk = a.y = ctypes.cast(buf, ctypes.c_void_p)
    a.batch, a.cin, a.cout, a.H, a.W = 1, 8, 8, 4, 4
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd_ex(ctypes.byref(a), -2, None) == -1
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd_ex(ctypes.byref(a), -1000, None) == -1
    for grid in (-1, 0, 1, 3):
        assert hip_lib.occd_wino_conv3x3_f16x2_fwd_ex(None, grid, None) == -1
    a.act = 7
    for grid in (-1, 0, 5):
        assert hip_lib.occd_wino_conv3x3_f16x2_fwd_ex(ctypes.byref(a), grid, None) == -1


def test_persist_switch_parses():
    from occdepth_amd import hip
    assert hip._parse_wino_persist("1") is True and hip._parse_wino_persist("0") is False
    for bad in ("", "2", "yes", "-1", "01"):
        with pytest.raises(ValueError):
            hip._parse_wino_persist(bad)
    assert isinstance(hip.WINO_PERSIST, bool)


def test_max_workgroups_needs_the_split_operand():
    """A K10 (float32) operand has no grid to choose: the argument is refused, not ignored."""
    from occdepth_amd import hip
    x, upk = torch.zeros(1, 8, 4, 4), torch.zeros(1)
    with pytest.raises(RuntimeError, match="max_workgroups"):
        hip.conv2d_3x3_fused(x, upk, 8, max_workgroups=0)
