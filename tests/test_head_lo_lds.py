"""K2s3h (csrc/conv3d_c32p.hip conv3d_c32_slide_f16x2_kernel) with the lo weight image resident in LDS beside hi and
hs = hi 2^-11 formed in registers (hip.set_head_lo(1), the default) against the form before, lo streamed from L2 through the
register ring beside the stored hi | hs images (set_head_lo(0)).  Both feed the same operands to the same MFMAs in the same
order -- the packer's stored hs is fp16(float(hi) 2^-11), the register product rounds the same way -- so every output must
be BIT-identical: every K2s3 geometry x six epilogues, a captured graph replayed twice, and the switch itself."""
import ctypes

import pytest
import torch

from test_bf16_conv import SLIDE_X3_CASES, vox_of

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from occdepth_amd import hip as h
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    h.load()
    return h


def _zero_vox(hip, B, dims, C):
    cs = -(-C // 8) * 8
    return hip.Vox(torch.zeros((B,) + tuple(dims) + (cs,), dtype=torch.float32, device=DEV), C)


def _both_forms(hip, launch, make_out):
    """`launch(out)` once with the ring (0) and once with the resident lo image (1); the whole output buffers."""
    bufs = {}
    for form in (0, 1):
        old = hip.set_head_lo(form)
        try:
            out = make_out()
            with hip.profile() as prof:
                launch(out)
            assert any(k.startswith("conv3d_c32x3") for k in prof.rows), prof.rows.keys()
            torch.cuda.synchronize()
            bufs[form] = out.buf
        finally:
            hip.set_head_lo(old)
    return bufs[0], bufs[1]


@pytest.mark.parametrize("case", SLIDE_X3_CASES)
def test_head_lo_lds_bit_identical_to_ring(hip, case):
    """Every geometry of SLIDE_X3_CASES (Z = 32 and the z-halo forms, D = 1 / 2 / 3, ragged channels and Y, batch 2, runs of a
    single plane, the six-row tile) with each epilogue of test_f16x2_head_kernel_accuracy plus input ReLU alone and a ragged
    cout_store: torch.equal between the two forms."""
    from occdepth_amd.fused import _pad_bias
    B, cin, cout, dims, d = case
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + d)
    x = torch.randn(B, cin, *dims, generator=g)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    vx = vox_of(hip, x, torch.float32)
    v1 = vox_of(hip, torch.randn(B, cout, *dims, generator=g), torch.float32)
    v2 = vox_of(hip, torch.randn(B, cout, *dims, generator=g), torch.float32)
    c2 = max(1, cout - 10)                         # ragged cout_store: 24 of 32 stored channels (22 -> 16, 2 -> 8)
    variants = [
        ("plain", cout, {}),
        ("relu_in", cout, dict(act_in=hip.ACT_RELU)),
        ("res1_relu", cout, dict(res1=v1, act_out=hip.ACT_RELU)),
        ("res1_res2_relu_in_out", cout, dict(res1=v1, res2=v2, act_in=hip.ACT_RELU, act_out=hip.ACT_RELU)),
        ("res2_only_relu_pre", cout, dict(res2=v2, act_out=hip.ACT_RELU_PRE)),
        ("ragged_cout_store", c2, {}),
    ]
    geo = dict(dilation=(d,) * 3, padding=(d,) * 3)
    for name, co, kw in variants:
        wpk, bpad = hip.pack_weights_f16x2(w[:co].contiguous()), _pad_bias(bias[:co].contiguous(), co)
        ring, lds = _both_forms(hip, lambda out: hip.conv3d_f16x2(vx, wpk, bpad, co, (3, 3, 3), out, **geo, **kw),
                                lambda: _zero_vox(hip, B, dims, co))
        assert torch.isfinite(ring).all() and float(ring.abs().max()) > 0, (case, name)
        assert torch.equal(ring, lds), (case, name, float((ring - lds).abs().max()))


def test_head_lo_lds_graph_replay_equals_eager(hip):
    """One launch captured into a graph and replayed twice equals the eager result: the work list's self-re-arming counters
    are untouched by the new form."""
    from occdepth_amd.fused import _pad_bias
    B, cin, cout, dims, d = 1, 32, 32, (16, 256, 32), 2
    g = torch.Generator().manual_seed(41)
    vx = vox_of(hip, torch.randn(B, cin, *dims, generator=g), torch.float32)
    v1 = vox_of(hip, torch.randn(B, cout, *dims, generator=g), torch.float32)
    wpk = hip.pack_weights_f16x2((torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5).to(DEV))
    bpad = _pad_bias(torch.randn(cout, generator=g).to(DEV), cout)
    out = _zero_vox(hip, B, dims, cout)

    def launch():
        hip.conv3d_f16x2(vx, wpk, bpad, cout, (3, 3, 3), out, dilation=(d,) * 3, padding=(d,) * 3, res1=v1,
                         act_out=hip.ACT_RELU)

    assert hip.set_head_lo(1) == 1                                     # the default form
    launch()                                                           # eager (also: one-time launch state before the capture)
    torch.cuda.synchronize()
    eager = out.buf.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        out.buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.buf, eager)
    launch()                                                           # and an eager launch after the replays
    torch.cuda.synchronize()
    assert torch.equal(out.buf, eager)


def test_head_lo_setter_contract(hip):
    """0 / 1 only: the wrapper refuses anything else and leaves the setting alone; the C entry point answers a value outside
    0..1 by restoring the default (1); every call returns the previous setting."""
    from occdepth_amd import abi
    lib = hip.load()
    assert abi.EXPORTS["occd_conv3d_head_set_lo"] == (ctypes.c_int32, [ctypes.c_int32])
    first = hip.set_head_lo(0)
    try:
        assert hip.set_head_lo(1) == 0
        assert hip.set_head_lo(0) == 1
        for bad in (2, -1, 7, True, 1.0, "1", None):
            with pytest.raises(ValueError):
                hip.set_head_lo(bad)
        assert hip.set_head_lo(0) == 0                                  # a refused value changed nothing
        assert lib.occd_conv3d_head_set_lo(7) == 0                      # out of range: the default comes back
        assert lib.occd_conv3d_head_set_lo(-3) == 1
        assert hip.set_head_lo(1) == 1
    finally:
        hip.set_head_lo(first if first in (0, 1) else 1)
    assert first == 1                                                   # the resident lo image is the default
