"""K2s3h (csrc/conv3d_c32p.hip conv3d_c32_slide_f16x2_kernel): the full-resolution head convolutions with the two-term fp16
split x = hi + 2^-11 lo' of both operands (three v_mfma_f32_32x32x16_f16 per K step), the default head split of the eval
path (fused.HEAD_SPLIT = "f16x2").  Accuracy against ATen float64 next to the exact-fp32 K2s and the bf16x3 K2s3 on the same
operands, range, non-finite contract, determinism and the model-level figures on the config-2 golden frame."""
import pytest
import torch
import torch.nn.functional as F

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


def _errs(out, ref):
    got = out.ncdhw().cpu().double()
    scale = ref.abs().max()
    return float((got - ref).abs().max() / scale), float((got - ref).norm() / ref.norm())


def _run_three(hip, x, w, bias, d, kw, ref, scale=None, label=""):
    """(f16x2, fp32 K2s, bf16x3 K2s3) errors against `ref` on the same operands; asserts the f16x2 launch took K2s3h."""
    from occdepth_amd.fused import _pad_bias
    B, cout, dims = x.shape[0], w.shape[0], tuple(x.shape[2:])
    vx = vox_of(hip, x, torch.float32)
    wd = w.to(DEV)
    sc = scale.to(DEV) if scale is not None else None
    bpad = _pad_bias(bias.to(DEV), cout)
    geo = dict(dilation=(d,) * 3, padding=(d,) * 3)
    res = {}
    for name in ("f16x2", "fp32", "bf16x3"):
        out = hip.Vox.empty(B, dims, cout, DEV)
        if name == "f16x2":
            with hip.profile() as prof:
                hip.conv3d_f16x2(vx, hip.pack_weights_f16x2(wd, sc), bpad, cout, (3, 3, 3), out, **geo, **kw)
            assert any(k.startswith("conv3d_c32x3") for k in prof.rows), prof.rows.keys()
        elif name == "fp32":
            hip.conv3d(vx, hip.pack_weights(wd, sc), bpad, cout, (3, 3, 3), out, **geo, **kw)
        else:
            hip.conv3d_bf16(vx, hip.pack_weights_bf16(wd, sc, split3=True), bpad, cout, (3, 3, 3), out, split3=True, **geo, **kw)
        res[name] = _errs(out, ref)
    (e, r), (e32, r32), (e3, r3) = res["f16x2"], res["fp32"], res["bf16x3"]
    print(f"K2s3h {label}: max err {e:.2e} (K2s fp32 {e32:.2e}, K2s3 bf16x3 {e3:.2e}), "
          f"rms {r:.2e} (K2s fp32 {r32:.2e}, K2s3 bf16x3 {r3:.2e})")
    return e, r, e32, r32


def _gate(e, r, e32, r32, what):
    assert e <= 4e-6, (what, e)
    assert e <= 2.0 * e32 + 1e-7 and r <= 2.0 * r32, (what, e, e32, r, r32)


@pytest.mark.parametrize("case", SLIDE_X3_CASES)
def test_f16x2_head_kernel_accuracy(hip, case):
    """Every K2s3 geometry and the four epilogue variants of test_conv3d_slide_x3_head_kernel: max error <= 4e-6 of the output
    maximum, max and rms error within 2x of the exact-fp32 K2s kernel's."""
    B, cin, cout, dims, d = case
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + d)
    x = torch.randn(B, cin, *dims, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5
    bias = torch.randn(cout, generator=g)
    r1 = torch.randn(B, cout, *dims, generator=g)
    r2 = torch.randn(B, cout, *dims, generator=g)
    base = F.conv3d(x.double(), w.double(), bias.double(), padding=d, dilation=d)
    base_relu_in = F.conv3d(F.relu(x).double(), w.double(), bias.double(), padding=d, dilation=d)
    v1, v2 = vox_of(hip, r1, torch.float32), vox_of(hip, r2, torch.float32)
    variants = [
        ("nres0", {}, base),
        ("nres1_relu", dict(res1=v1, act_out=hip.ACT_RELU), F.relu(base + r1.double())),
        ("nres2_relu_in", dict(res1=v1, res2=v2, act_in=hip.ACT_RELU, act_out=hip.ACT_RELU),
         F.relu(base_relu_in + r1.double() + r2.double())),
        ("res2_only_relu_pre", dict(res2=v2, act_out=hip.ACT_RELU_PRE), F.relu(base) + r2.double()),
    ]
    for name, kw, ref in variants:
        _gate(*_run_three(hip, x, w, bias, d, kw, ref, label=f"{case} {name}"), (case, name))


RANGE_CASE = (1, 32, 32, (16, 256, 32))


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("xs,ws,bn", [(-16, 0, False), (-8, 0, False), (8, 0, False), (0, -12, False), (0, 6, False),
                                      (0, 0, True)],
                         ids=["x2^-16", "x2^-8", "x2^+8", "w2^-12", "w2^+6", "bn_scale"])
def test_f16x2_range(hip, d, xs, ws, bn):
    """Activations scaled by 2^-16 / 2^-8 / 2^+8, weights by 2^-12 / 2^+6, and a BN-folded per-channel scale spanning six
    decades (the per-channel power-of-two weight scaling): the same 2x gate against the exact-fp32 kernel."""
    B, cin, cout, dims = RANGE_CASE
    g = torch.Generator().manual_seed(17 + d)
    x = torch.randn(B, cin, *dims, generator=g) * 2.0 ** xs
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5 * 2.0 ** ws
    bias = torch.randn(cout, generator=g) * 2.0 ** (xs + ws)
    scale = 10.0 ** torch.linspace(-4, 2, cout) if bn else None
    wref = w * scale.view(-1, 1, 1, 1, 1) if bn else w
    if bn:
        bias = bias * scale
    ref = F.conv3d(x.double(), wref.double(), bias.double(), padding=d, dilation=d)
    e, r, e32, r32 = _run_three(hip, x, w, bias, d, {}, ref, scale=scale, label=f"range x2^{xs} w2^{ws} bn={bn} d={d}")
    _gate(e, r, e32, r32, (xs, ws, bn, d))
    if bn:   # per output channel, relative to that channel's own maximum (a shared exponent would lose the small channels)
        from occdepth_amd.fused import _pad_bias
        vx = vox_of(hip, x, torch.float32)
        out = hip.Vox.empty(B, dims, cout, DEV)
        hip.conv3d_f16x2(vx, hip.pack_weights_f16x2(w.to(DEV), scale.to(DEV)), _pad_bias(bias.to(DEV), cout), cout, (3, 3, 3),
                         out, dilation=(d,) * 3, padding=(d,) * 3)
        got = out.ncdhw().cpu().double()
        per_ch = ((got - ref).abs().amax(dim=(0, 2, 3, 4)) / ref.abs().amax(dim=(0, 2, 3, 4))).max().item()
        print(f"bn_scale d={d}: worst per-channel max err {per_ch:.2e}")
        assert per_ch <= 4e-6, per_ch


def test_f16x2_subnormal_operands_through_the_mfma(hip):
    """Activations of 2^-22: after the 2^1 pre-scale every hi term is an fp16 SUBNORMAL (< 2^-14).  If the matrix pipe flushed
    fp16 denormal inputs the result would be (almost) zero; it must stay accurate to the subnormal spacing."""
    from occdepth_amd.fused import _pad_bias
    B, cin, cout, dims = RANGE_CASE
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, *dims, generator=g) * 2.0 ** -22
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5
    ref = F.conv3d(x.double(), w.double(), None, padding=1)
    vx = vox_of(hip, x, torch.float32)
    out = hip.Vox.empty(B, dims, cout, DEV)
    hip.conv3d_f16x2(vx, hip.pack_weights_f16x2(w.to(DEV)), _pad_bias(torch.zeros(cout, device=DEV), cout), cout, (3, 3, 3), out,
                     padding=(1, 1, 1))
    e, r = _errs(out, ref)
    print(f"subnormal hi terms: max err {e:.2e}, rms {r:.2e}")
    assert e < 1e-3 and r < 1e-4, (e, r)


def test_f16x2_non_finite_and_fp16_overflow(hip):
    """The bf16x3 contract (test_non_finite_inputs_split_poisons_exact_propagates), and the one range difference: a FINITE
    activation beyond the fp16 operand range (|x| >= 32760 with the 2^1 pre-scale; 40000 and -1e6 here) also makes every
    output it reaches non-finite -- never a plausible finite number -- and leaves every other output bit-identical."""
    from occdepth_amd.fused import _pad_bias
    B, cin, cout, dims, d = 1, 32, 32, (16, 256, 32), 1
    g = torch.Generator().manual_seed(99)
    x = torch.randn(B, cin, *dims, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (cin * 27) ** 0.5
    bias = torch.randn(cout, generator=g)
    wpk, bpad = hip.pack_weights_f16x2(w.to(DEV)), _pad_bias(bias.to(DEV), cout)

    def run(xin):
        out = hip.Vox.empty(B, dims, cout, DEV)
        hip.conv3d_f16x2(vox_of(hip, xin, torch.float32), wpk, bpad, cout, (3, 3, 3), out, dilation=(d,) * 3, padding=(d,) * 3)
        return out.ncdhw().cpu()

    clean = run(x)
    spots = [(5, 8, 100, 16), (9, 3, 30, 7), (2, 12, 200, 20)]
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
    # just below the operand range: finite and accurate
    xb = x.clone()
    xb[0, 5, 8, 100, 16] = 32000.0
    ref = F.conv3d(xb.double(), w.double(), bias.double(), padding=d, dilation=d)
    got = run(xb).double()
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max() / ref.abs().max()) < 4e-6


def test_f16x2_back_to_back_launches_are_bit_identical(hip):
    """The work list's self-re-arming counters: two consecutive launches compute the same bits."""
    from occdepth_amd.fused import _pad_bias
    for dims, d in (((16, 256, 32), 2), ((16, 128, 64), 1)):
        g = torch.Generator().manual_seed(3 + d)
        x = torch.randn(1, 32, *dims, generator=g)
        w = torch.randn(32, 32, 3, 3, 3, generator=g) / (32 * 27) ** 0.5
        vx = vox_of(hip, x, torch.float32)
        wpk, bpad = hip.pack_weights_f16x2(w.to(DEV)), _pad_bias(torch.randn(32, generator=g).to(DEV), 32)
        outs = []
        for _ in range(2):
            o = hip.Vox.empty(1, dims, 32, DEV)
            hip.conv3d_f16x2(vx, wpk, bpad, 32, (3, 3, 3), o, dilation=(d,) * 3, padding=(d,) * 3)
            outs.append(o.buf.clone())
        assert torch.equal(outs[0], outs[1])


def test_f16x2_rejects_non_head_geometry(hip):
    """dtype 3 has no generic kernel: a launch outside K2s3h's geometry is an error, not a silent fallback."""
    x = hip.Vox(torch.randn(1, 8, 8, 8, 32, device=DEV), 32)
    w = torch.randn(32, 32, 3, 3, 3, device=DEV)
    out = hip.Vox.empty(1, (8, 8, 8), 32, DEV)
    with pytest.raises(RuntimeError):
        hip.conv3d_f16x2(x, hip.pack_weights_f16x2(w), None, 32, (3, 3, 3), out, padding=(1, 1, 1))


def _elementwise(got, ref):
    m = ref.abs() >= 0.01 * ref.abs().max()
    return float(((got - ref).abs()[m] / ref.abs()[m]).max())


def test_f16x2_model_level_config2_golden(hip):
    """The config-2 golden frame (kitti_a100, eager) with OCCDEPTH_HEAD_SPLIT = f16x2 and = bf16x3: both within the golden
    bound (1e-3 of each output's maximum); the element-wise figure and the largest |x| that reaches a head launch (the margin
    below the fp16 operand limit of 32760) are printed."""
    import golden_cases as gc
    from test_parity_gpu import benched_batch, config2_errors, gold
    from test_oracle_vs_golden import build_product
    from occdepth_amd import fused
    saved = fused.HEAD_SPLIT
    real = hip.conv3d_f16x2
    seen = []

    def spy(x, *a, **kw):
        seen.append(float(x.buf[..., x.coff:x.coff + x.C].abs().max()))
        return real(x, *a, **kw)

    try:
        m, _, _ = build_product("kitti_a100")
        m = m.to(DEV).eval()
        batch = benched_batch()
        g = gold("occdepth_kitti_a100")
        for mode in ("f16x2", "bf16x3"):
            fused.set_head_split(mode)
            seen.clear()
            hip.conv3d_f16x2 = spy
            with torch.no_grad(), hip.profile() as prof:
                out = m(batch)
                torch.cuda.synchronize()
            hip.conv3d_f16x2 = real
            assert any(k.startswith("conv3d_c32x3") for k in prof.rows)
            worst = config2_errors(out)
            elem = {k: _elementwise(gc.subsample(v.cpu().contiguous()).double(), torch.from_numpy(g[k]).double())
                    for k, v in out.items() if k in ("ssc_logit", "occ_logit")}
            print(f"config-2 golden, head split {mode}: max rel {({k: f'{e:.2e}' for k, e in worst.items()})}, "
                  f"max_elementwise_rel_where_ref_ge_1pct_of_scale {({k: f'{e:.2e}' for k, e in elem.items()})}")
            if mode == "f16x2":
                print(f"K2s3h launches {len(seen)}, max |x| per launch {[f'{v:.3g}' for v in seen]} (operand limit 32760)")
                assert len(seen) >= 7 and max(seen) < 32760
            else:
                assert not seen
            assert max(worst.values()) < 1e-3, (mode, worst)
    finally:
        hip.conv3d_f16x2 = real
        fused.set_head_split(saved)
