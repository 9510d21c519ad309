"""K2bh (csrc/conv3d_bf16.hip, SPLIT = 2): the generic implicit-GEMM 3-D convolution with K2s3h's two-term fp16 split
(x' = hi + 2^-11 lo', three v_mfma_f32_32x32x16_f16 per K step, hs formed in registers), the default form of K2b's
float32-accurate launches in the eval path (fused.K2B_SPLIT = "f16x2"): the long-K 3x3x3 convolutions of small volumes and
the merged phase launches of the transposed convolutions.  Accuracy against ATen float64 next to the exact-fp32 K2 and the
bf16x3 K2b on the same operands, every tile variant, merged phases, range, the non-finite / overflow contract, determinism,
routing and the model-level figure."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from test_bf16_conv import FWD_CASES, fwd_tensors, vox_of

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    from occdepth_amd import hip as h
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    h.load()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    return h


def _errs(out, ref):
    got = out.ncdhw().cpu().double()
    return float((got - ref).abs().max() / ref.abs().max()), float((got - ref).norm() / ref.norm())


def _gate(e, r, e32, r32, what):
    """The head test's gate (tests/test_head_f16x2.py)."""
    assert e <= 4e-6, (what, e)
    assert e <= 2.0 * e32 + 1e-7 and r <= 2.0 * r32, (what, e, e32, r, r32)


def _run_three(hip, x, w, bias, geo, kw, ref, scale=None, label="", tile_hint=0, x3=True):
    """(f16x2 K2bh, exact-fp32 K2, bf16x3 K2b) on the same operands against `ref`; returns (e, r, e32, r32, K2bh's Vox)."""
    from occdepth_amd.fused import _pad_bias
    B, cout = x.shape[0], w.shape[0]
    k = tuple(w.shape[2:])
    odims = tuple(ref.shape[2:])
    vx = vox_of(hip, x, torch.float32)
    wd = w.to(DEV)
    sc = scale.to(DEV) if scale is not None else None
    bpad = _pad_bias(bias.to(DEV), cout) if bias is not None else None
    res, keep = {}, None
    for name in ("f16x2", "fp32", "bf16x3") if x3 else ("f16x2", "fp32"):
        out = hip.Vox.empty(B, odims, cout, DEV)
        if name == "f16x2":
            with hip.profile() as prof:
                hip.conv3d_bf16(vx, hip.pack_weights_f16x2(wd, sc), bpad, cout, k, out, f16x2=True, tile_hint=tile_hint, **geo, **kw)
            assert any(t.startswith("conv3d_bf16x3_f16x2") for t in prof.rows), prof.rows.keys()
            keep = out
        elif name == "fp32":
            hip.conv3d(vx, hip.pack_weights(wd, sc), bpad, cout, k, out, **geo, **kw)
        else:
            hip.conv3d_bf16(vx, hip.pack_weights_bf16(wd, sc, split3=True), bpad, cout, k, out, split3=True, tile_hint=tile_hint,
                            **geo, **kw)
        res[name] = _errs(out, ref)
    (e, r), (e32, r32) = res["f16x2"], res["fp32"]
    e3, r3 = res.get("bf16x3", (float("nan"), float("nan")))
    print(f"K2bh {label}: max err {e:.2e} (K2 fp32 {e32:.2e}, K2b bf16x3 {e3:.2e}), "
          f"rms {r:.2e} (K2 fp32 {r32:.2e}, K2b bf16x3 {r3:.2e}), rms ratio to K2 {r / r32:.2f}")
    return e, r, e32, r32, keep


ACC_CASES = ["aspp_256", "aspp_256_full_d3", "cin_144_splitk", "k3_s2", "classes_34_20", "ragged_5_20", "nyu_z15", "dec_80_80"]


@pytest.mark.parametrize("name", ACC_CASES)
def test_k2bh_accuracy_vs_float64(hip, name):
    """Against ATen float64 on the UN-rounded operands, residual + output ReLU as test_conv3d_bf16x3_reaches_float32_accuracy
    and a second pass with the input ReLU: max error <= 4e-6 of the output maximum, max and rms within 2x of the exact-fp32
    K2's; the padding channels of `out` are zero."""
    B, cin, cout, dims, k, s, p, d = FWD_CASES[name]
    x, w, b, r1, odims = fwd_tensors(name)
    geo = dict(stride=s, dilation=d, padding=p)
    v1 = vox_of(hip, r1, torch.float32)
    ref = F.relu(F.conv3d(x.double(), w.double(), b.double(), stride=s, padding=p, dilation=d) + r1.double())
    *g, out = _run_three(hip, x, w, b, geo, dict(res1=v1, act_out=hip.ACT_RELU), ref, label=name)
    _gate(*g, name)
    if out.cs > cout:
        assert float(out.buf[..., cout:].abs().max()) == 0.0
    ref2 = F.relu(F.conv3d(F.relu(x.double()), w.double(), b.double(), stride=s, padding=p, dilation=d) + r1.double())
    *g, out = _run_three(hip, x, w, b, geo, dict(res1=v1, act_in=hip.ACT_RELU, act_out=hip.ACT_RELU), ref2, label=name + " relu_in")
    _gate(*g, (name, "relu_in"))
    if out.cs > cout:
        assert float(out.buf[..., cout:].abs().max()) == 0.0


@pytest.mark.parametrize("hint", [2, 3, 5, 7, 8, 9])
def test_k2bh_all_variants(hip, hint):
    """tile_hint 2, 3, 5, 7, 8, 9 = variants 1, 2, 4, 6, 7 and the split-K variant 8: every SPLIT = 2 instantiation, on the shape
    of test_conv3d_bf16_all_variants (ragged channels, dilation 2)."""
    torch.manual_seed(hint)
    B, cin, cout, dims = 1, 40, 136, (5, 7, 12)
    x = torch.randn(B, cin, *dims)
    w = torch.randn(cout, cin, 3, 3, 3) / (cin * 27) ** 0.5
    ref = F.conv3d(x.double(), w.double(), None, padding=2, dilation=2)
    *g, out = _run_three(hip, x, w, None, dict(dilation=(2, 2, 2), padding=(2, 2, 2)), {}, ref, label=f"hint {hint}", tile_hint=hint)
    _gate(*g, hint)


PHASE_CASES = [(2, 128, 64, (8, 8, 4)), (1, 64, 32, (16, 12, 8)), (1, 40, 20, (5, 3, 5)), (1, 256, 128, (8, 8, 2))]


def _phase_setup(hip, case):
    from test_hip_vs_aten import randomize_bn
    B, cin, cout, dims = case
    torch.manual_seed(cin)
    convt = nn.ConvTranspose3d(cin, cout, 3, stride=2, padding=1, output_padding=1).to(DEV)
    bn = randomize_bn(nn.BatchNorm3d(cout)).to(DEV).eval()
    x = torch.randn(B, cin, *dims, device=DEV)
    res = torch.randn(B, cout, *(2 * n for n in dims), device=DEV)
    return convt, bn, x, res


@pytest.mark.parametrize("case", PHASE_CASES)
def test_k2bh_merged_phases(hip, case):
    """The cases of test_transposed_conv_phases_one_launch_equals_eight through fused.ConvTransposePlan with the switch on
    f16x2 (one K2bh launch) and on bf16x3 (bit for bit the explicit split3 launch); error against the float64 transposed
    convolution + BatchNorm + residual + ReLU below max(2e-6, 1.5 e_K2), the bound of the existing test."""
    from occdepth_amd import fused
    from test_hip_vs_aten import rel_err
    B, cin, cout, dims = case
    convt, bn, x, res = _phase_setup(hip, case)
    saved = (fused.PHASES_ONE_LAUNCH, fused.PHASES_X3, fused.K2B_SPLIT)
    with torch.no_grad():
        plan = fused.ConvTransposePlan(convt, bn)
        vx, vr = hip.Vox.from_ncdhw(x), hip.Vox.from_ncdhw(res)
        try:
            fused.PHASES_ONE_LAUNCH, fused.PHASES_X3 = True, True
            fused.set_k2b_split("f16x2")
            with hip.profile() as prof:
                one_h = plan(vx, res1=vr, act_out=hip.ACT_RELU).ncdhw()
            assert any(t.startswith("conv3d_bf16x3_phases_f16x2") for t in prof.rows), list(prof.rows)
            fused.set_k2b_split("bf16x3")
            with hip.profile() as prof:
                one_3 = plan(vx, res1=vr, act_out=hip.ACT_RELU).ncdhw()
            convs = [t for t in prof.rows if t.startswith("conv3d")]
            assert convs and all(t.startswith("conv3d_bf16x3_phases") and "f16x2" not in t for t in convs), convs
            out = hip.Vox.empty(B, tuple(2 * n for n in dims), cout, DEV)
            hip.conv3d_phases(vx, [(wpk.image("x3"), kern, off) for off, kern, _, wpk in plan._phases], plan._bias, cout, out, res1=vr,
                              act_out=hip.ACT_RELU, out_pos=vx.dims, o_stride=(2, 2, 2), split3=True)
            assert torch.equal(one_3, out.ncdhw())
            fused.PHASES_X3 = False
            one_k2 = plan(vx, res1=vr, act_out=hip.ACT_RELU).ncdhw()
        finally:
            fused.PHASES_ONE_LAUNCH, fused.PHASES_X3 = saved[:2]
            fused.set_k2b_split(saved[2])
    ref64 = F.relu(bn.double()(F.conv_transpose3d(x.double(), convt.weight.double(), convt.bias.double(), stride=2, padding=1,
                                                  output_padding=1)) + res.double())
    bn.float()
    e_h, e_3, e_k2 = rel_err(one_h.double(), ref64), rel_err(one_3.double(), ref64), rel_err(one_k2.double(), ref64)
    print(case, f"vs float64: K2bh f16x2 {e_h:.2e}, K2b bf16x3 {e_3:.2e}, K2 exact fp32 {e_k2:.2e}")
    assert e_h < max(2e-6, 1.5 * e_k2), (e_h, e_k2)
    assert e_3 < max(2e-6, 1.5 * e_k2), (e_3, e_k2)


# long-K shapes only (K = 3888 and 6912): with few products (K = 135) and activations x 2^-16 the hi terms are subnormal and
# the rms is 2.5x the comparator's in a CPU emulation of the scheme; the routed launches have K >= 3456 or run at natural scale
RANGE_SHAPES = {
    "k3888": (2, 144, 128, (6, 10, 4), 1),
    "aspp_256": FWD_CASES["aspp_256"][:4] + (2,),
}


@pytest.mark.parametrize("shape", list(RANGE_SHAPES))
@pytest.mark.parametrize("xs,ws,bn", [(-16, 0, False), (-8, 0, False), (8, 0, False), (0, -12, False), (0, 6, False),
                                      (0, 0, True)],
                         ids=["x2^-16", "x2^-8", "x2^+8", "w2^-12", "w2^+6", "bn_scale"])
def test_k2bh_range(hip, shape, xs, ws, bn):
    """The rows of test_f16x2_range: activations x 2^-16 / 2^-8 / 2^+8, weights x 2^-12 / 2^+6, a per-channel scale over six
    decades (per-channel error <= 4e-6 of that channel's own maximum); the same 2x gate against the exact-fp32 K2."""
    B, cin, cout, dims, d = RANGE_SHAPES[shape]
    g = torch.Generator().manual_seed(17 + d + cin)
    x = torch.randn(B, cin, *dims, generator=g) * 2.0 ** xs
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5 * 2.0 ** ws
    bias = torch.randn(cout, generator=g) * 2.0 ** (xs + ws)
    scale = 10.0 ** torch.linspace(-4, 2, cout) if bn else None
    wref = w * scale.view(-1, 1, 1, 1, 1) if bn else w
    if bn:
        bias = bias * scale
    ref = F.conv3d(x.double(), wref.double(), bias.double(), padding=d, dilation=d)
    e, r, e32, r32, out = _run_three(hip, x, w, bias, dict(dilation=(d,) * 3, padding=(d,) * 3), {}, ref, scale=scale,
                                     label=f"range {shape} x2^{xs} w2^{ws} bn={bn}", x3=False)
    _gate(e, r, e32, r32, (shape, xs, ws, bn))
    if bn:
        got = out.ncdhw().cpu().double()
        per_ch = ((got - ref).abs().amax(dim=(0, 2, 3, 4)) / ref.abs().amax(dim=(0, 2, 3, 4))).max().item()
        print(f"bn_scale {shape}: worst per-channel max err {per_ch:.2e}")
        assert per_ch <= 4e-6, per_ch


def test_k2bh_non_finite_and_fp16_overflow(hip):
    """The contract of test_f16x2_non_finite_and_fp16_overflow on the generic kernel (the split-K variant: the poison also
    crosses the K groups' sum): +-Inf, NaN and finite activations beyond the fp16 operand range (|x| >= 32760) make exactly
    the outputs they reach non-finite and leave every other output bit-identical; 32000 stays finite and accurate."""
    from occdepth_amd.fused import _pad_bias
    B, cin, cout, dims, d = 1, 128, 128, (6, 10, 4), 1
    g = torch.Generator().manual_seed(99)
    x = torch.randn(B, cin, *dims, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5
    bias = torch.randn(cout, generator=g)
    wpk, bpad = hip.pack_weights_f16x2(w.to(DEV)), _pad_bias(bias.to(DEV), cout)

    def run(xin):
        out = hip.Vox.empty(B, dims, cout, DEV)
        hip.conv3d_bf16(vox_of(hip, xin, torch.float32), wpk, bpad, cout, (3, 3, 3), out, dilation=(d,) * 3, padding=(d,) * 3,
                        f16x2=True)
        return out.ncdhw().cpu()

    clean = run(x)
    spots = [(5, 0, 3, 1), (100, 3, 9, 3), (64, 5, 0, 0)]
    ones = torch.ones(cout, cin, 3, 3, 3)
    for vals in ((float("inf"), float("-inf"), float("nan")), (40000.0, -1e6, 32768.0)):
        xp = x.clone()
        mask = torch.zeros_like(x)
        for (c, i, j, k), v in zip(spots, vals):
            xp[0, c, i, j, k] = v
            mask[0, c, i, j, k] = 1.0
        reached = F.conv3d(mask, ones, padding=d, dilation=d) > 0
        got = run(xp)
        assert torch.equal(~torch.isfinite(got), reached), vals
        assert torch.equal(got[~reached], clean[~reached]), vals
    xb = x.clone()
    xb[0, 5, 0, 3, 1] = 32000.0
    ref = F.conv3d(xb.double(), w.double(), bias.double(), padding=d, dilation=d)
    got = run(xb).double()
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max() / ref.abs().max()) < 4e-6


def test_k2bh_back_to_back_launches_are_bit_identical(hip):
    """Variant 8 (the K groups are summed through LDS in a fixed order) and a merged phase launch: two consecutive launches
    compute the same bits."""
    from occdepth_amd import fused
    from occdepth_amd.fused import _pad_bias
    B, cin, cout, dims, k, s, p, d = FWD_CASES["aspp_256"]
    x, w, b, r1, odims = fwd_tensors("aspp_256")
    vx = vox_of(hip, x, torch.float32)
    wpk, bpad = hip.pack_weights_f16x2(w.to(DEV)), _pad_bias(b.to(DEV), cout)
    outs = []
    for _ in range(2):
        o = hip.Vox.empty(B, odims, cout, DEV)
        hip.conv3d_bf16(vx, wpk, bpad, cout, k, o, dilation=d, padding=p, f16x2=True, tile_hint=9)
        outs.append(o.buf.clone())
    assert torch.equal(outs[0], outs[1])
    convt, bn, xt, res = _phase_setup(hip, PHASE_CASES[0])
    saved = fused.K2B_SPLIT
    try:
        fused.set_k2b_split("f16x2")
        with torch.no_grad():
            plan = fused.ConvTransposePlan(convt, bn)
            vt, vr = hip.Vox.from_ncdhw(xt), hip.Vox.from_ncdhw(res)
            with hip.profile() as prof:
                a = plan(vt, res1=vr, act_out=hip.ACT_RELU).buf.clone()
            assert any(t.startswith("conv3d_bf16x3_phases_f16x2") for t in prof.rows), list(prof.rows)
            b2 = plan(vt, res1=vr, act_out=hip.ACT_RELU).buf.clone()
    finally:
        fused.set_k2b_split(saved)
    assert torch.equal(a, b2)


def _conv_bn(cin, cout, seed, **kw):
    from test_hip_vs_aten import randomize_bn
    torch.manual_seed(seed)
    conv = nn.Conv3d(cin, cout, 3, bias=False, **kw).to(DEV)
    bn = randomize_bn(nn.BatchNorm3d(cout), seed).to(DEV).eval()
    return conv, bn


def _conv_tags(prof):
    return [t for t in prof.rows if t.startswith("conv3d")]


@pytest.mark.parametrize("geom", ["d1", "d2", "d3", "s2_512"])
def test_k2bh_routing(hip, geom):
    """ConvPlan on the CRP's small-volume convolutions (256 -> 256 dilated at (8, 8, 4), 256 -> 512 stride 2): the default
    switch takes K2bh, set_k2b_split("bf16x3") the bf16x3 kernel with exactly the bits of an explicit split3 launch, and a
    weight with one Inf keeps bf16x3."""
    from occdepth_amd import fused
    d = {"d1": 1, "d2": 2, "d3": 3}.get(geom, 1)
    kw = dict(padding=d, dilation=d) if geom != "s2_512" else dict(padding=1, stride=2)
    cout = 512 if geom == "s2_512" else 256
    conv, bn = _conv_bn(256, cout, 7 + d, **kw)
    x = torch.randn(1, 256, 8, 8, 4, device=DEV)
    vx = hip.Vox.from_ncdhw(x)
    saved = fused.K2B_SPLIT
    try:
        with torch.no_grad():
            plan = fused.ConvPlan(conv, bn)
            fused.set_k2b_split("f16x2")
            with hip.profile() as prof:
                got_h = plan(vx, act_out=hip.ACT_RELU)
            assert [t for t in _conv_tags(prof) if t.startswith("conv3d_bf16x3_f16x2")], list(prof.rows)
            fused.set_k2b_split("bf16x3")
            with hip.profile() as prof:
                got_3 = plan(vx, act_out=hip.ACT_RELU)
            tags = _conv_tags(prof)
            assert tags and all(t.startswith("conv3d_bf16x3") and "f16x2" not in t for t in tags), tags
            k, s, dl, p = plan.geometry()
            out = hip.Vox.empty(1, plan.out_dims(vx.dims), cout, DEV)
            hip.conv3d_bf16(vx, plan._wpk.image("x3"), plan._bias, cout, k, out, stride=s, dilation=dl, padding=p, act_out=hip.ACT_RELU,
                            split3=True)
            assert torch.equal(got_3.buf, out.buf)
            y = F.conv3d(x.double(), conv.weight.double(), None, stride=conv.stride, padding=conv.padding, dilation=conv.dilation)
            ref = F.relu(F.batch_norm(y, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(),
                                      False, 0.0, bn.eps))
            e_h, e_3 = _errs(got_h, ref.cpu())[0], _errs(got_3, ref.cpu())[0]
            print(f"routing {geom}: K2bh {e_h:.2e}, bf16x3 {e_3:.2e}")
            assert e_h <= 4e-6
            # one Inf weight: no power-of-two scale, the plan keeps bf16x3
            fused.set_k2b_split("f16x2")
            conv.weight[3, 5, 1, 1, 1] = float("inf")             # (in place: the plan's stamp sees the new version)
            with hip.profile() as prof:
                plan(vx, act_out=hip.ACT_RELU)
            tags = _conv_tags(prof)
            assert tags and all(t.startswith("conv3d_bf16x3") and "f16x2" not in t for t in tags), tags
    finally:
        fused.set_k2b_split(saved)


def test_k2bh_switch_leaves_other_routes_alone(hip):
    """A head-geometry launch (K2s3h / K2s3 under OCCDEPTH_HEAD_SPLIT) and a small volume that is not 3x3x3 take the same
    kernel and compute the same bits under both values of the switch."""
    from occdepth_amd import fused
    saved = fused.K2B_SPLIT
    torch.manual_seed(21)
    head = nn.Conv3d(32, 32, 3, padding=1, bias=False).to(DEV)
    xh = hip.Vox.from_ncdhw(torch.randn(1, 32, 16, 256, 32, device=DEV))
    k131 = nn.Conv3d(256, 128, (1, 3, 1), padding=(0, 1, 0), bias=False).to(DEV)
    xs = hip.Vox.from_ncdhw(torch.randn(1, 256, 8, 8, 4, device=DEV))
    try:
        with torch.no_grad():
            for conv, vx in ((head, xh), (k131, xs)):
                outs, tags = [], []
                for mode in ("f16x2", "bf16x3"):
                    fused.set_k2b_split(mode)
                    plan = fused.ConvPlan(conv)
                    with hip.profile() as prof:
                        outs.append(plan(vx).buf.clone())
                    tags.append(sorted(_conv_tags(prof)))
                assert tags[0] == tags[1] and not any("bf16x3_f16x2" in t for t in tags[0]), tags
                assert torch.equal(outs[0], outs[1])
    finally:
        fused.set_k2b_split(saved)


def test_k2bh_rejects_wrong_operands(hip):
    """f16x2=True takes the uint8 image of pack_weights_f16x2 and float32 tensors; anything else raises."""
    x = hip.Vox(torch.randn(1, 8, 8, 4, 128, device=DEV), 128)
    w = torch.randn(128, 128, 3, 3, 3, device=DEV)
    out = hip.Vox.empty(1, (8, 8, 4), 128, DEV)
    with pytest.raises(RuntimeError):
        hip.conv3d_bf16(x, hip.pack_weights_bf16(w, split3=True), None, 128, (3, 3, 3), out, padding=(1, 1, 1), f16x2=True)
    xb = hip.Vox(x.buf.to(torch.bfloat16), 128)
    outb = hip.Vox.empty(1, (8, 8, 4), 128, DEV, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        hip.conv3d_bf16(xb, hip.pack_weights_f16x2(w), None, 128, (3, 3, 3), outb, padding=(1, 1, 1), f16x2=True)


def test_k2bh_model_level_unet3d(hip):
    """tests/test_hip_vs_aten.py's kitti_ps2 UNet3D eval forward with the switch on each value against ATen (< 2e-4 of each
    output's maximum); the distance between the two forms is printed per output."""
    from occdepth_amd import fused
    from occdepth_amd.models.unet3d_kitti import UNet3D
    from test_hip_vs_aten import aten_reference, compare, randomize_bn
    torch.manual_seed(2)
    m = UNet3D(20, nn.BatchNorm3d, (64, 64, 16), 16, 2, context_prior=True, cascade_cls=True, occluded_cls=False)
    x = torch.randn(1, 16, 32, 32, 8, device=DEV)
    m = randomize_bn(m).to(DEV).eval()
    saved = fused.K2B_SPLIT
    outs = {}
    try:
        for mode in ("f16x2", "bf16x3"):
            fused.set_k2b_split(mode)
            with torch.no_grad(), hip.profile() as prof:
                outs[mode] = m({"x3d": x})
            has = any("bf16x3_f16x2" in t or "phases_f16x2" in t for t in prof.rows)
            assert has == (mode == "f16x2"), (mode, list(prof.rows))
    finally:
        fused.set_k2b_split(saved)
    ref = aten_reference(m, {"x3d": x})

    def dist(a, b, what):
        if isinstance(b, dict):
            for k in b:
                dist(a[k], b[k], f"{what}.{k}")
        elif isinstance(b, (tuple, list)):
            for i, (p, q) in enumerate(zip(a, b)):
                dist(p, q, f"{what}[{i}]")
        else:
            print(f"{what}: max |f16x2 - bf16x3| / max |bf16x3| = {float((a - b).abs().max() / b.abs().max()):.2e}")

    dist(outs["f16x2"], outs["bf16x3"], "kitti_ps2")
    for mode in ("f16x2", "bf16x3"):
        compare(outs[mode], ref, 2e-4, f"kitti_ps2 {mode}")
