"""K10h: the fused Winograd F(2x2, 3x3) convolution on the two-term fp16 split (csrc/wino_conv2d.hip, fused.WINO_SPLIT = "f16x2").

Reference: ATen float64 conv2d + affine + activation (+ residual) on the CPU.  Two gates per case, K10h and K10 on the SAME
inputs:  max |err| / max |ref| < 2e-5 (the tolerance of K10's own GPU test)  and  rms err (K10h) <= 2 x rms err (K10).
Without a GPU the same gates run on a torch emulation of both kernels' arithmetic (pack scaling, staging factor, the three-term
sum in float32, the epilogue factor).
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from test_winograd2d import FUSED_CASES

# (B, Cin, Cout, H, W, act, residual, res_first, tile_hint)
EXTRA_CASES = [
    (1, 16, 32, 4, 6, None, False, False, 0),         # exactly one 16-cin step, one cout block
    (1, 17, 33, 4, 6, None, False, False, 0),         # one channel past a step and past a cout block
    (1, 48, 96, 9, 35, "leaky", False, False, 0),     # three steps, three cout blocks
]
CASES = list(FUSED_CASES) + EXTRA_CASES
RANGE_GEOM = (2, 64, 64, 24, 77, "relu", True, True, 0)
# (activation scale, weight scale, BatchNorm scale spread in decades)
RANGES = [(2.0 ** -16, 0.1, 0), (2.0 ** -8, 0.1, 0), (2.0 ** 8, 0.1, 0), (1.0, 2.0 ** -12, 0), (1.0, 2.0 ** 6, 0), (1.0, 0.1, 6)]
STAGE = 2.0                    # kWinoStageExp = 1
OVERFLOW_AT = 8190.0           # fp16(2 * 4 |x|) rounds to Inf from 65520 on

Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1.]])
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1.]], dtype=torch.float64)
At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1.]], dtype=torch.float64)
ACT = {"leaky": lambda t: F.leaky_relu(t, 0.01), "relu": F.relu, "swish": lambda t: t * torch.sigmoid(t), None: lambda t: t}


def make(case, xs=1.0, ws=0.1, decades=0):
    B, cin, cout, H, W, act, with_res, res_first, hint = case
    g = torch.Generator().manual_seed(B * 1000 + cin + H + hint)
    x = torch.randn(B, cin, H, W, generator=g) * xs
    w = torch.randn(cout, cin, 3, 3, generator=g) * ws
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    if decades:
        scale = scale * torch.pow(10.0, torch.linspace(-decades / 2, decades / 2, cout))
    # shift and residual at the scale of the convolution's output, so that they do not hide its error
    mag = xs * ws * 3.0 * cin ** 0.5
    shift = shift * mag * scale
    res = torch.randn(B, cout, H, W, generator=g) * mag if with_res else None
    return x, w, scale, shift, res


def reference(case, x, w, scale, shift, res):
    act, with_res, res_first = case[5], case[6], case[7]
    ref = F.conv2d(x.double(), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if with_res and res_first:
        ref = ref + res.double()
    ref = ACT[act](ref)
    if with_res and not res_first:
        ref = ref + res.double()
    return ref


def errors(y, ref):
    d = y.double().cpu() - ref
    s = float(ref.abs().max())
    return float(d.abs().max()) / s, float(d.pow(2).mean().sqrt()) / s


def check_gates(tag, e_split, e_f32):
    ratio = e_split[1] / e_f32[1]
    print(tag, "K10h max/rms %.2e %.2e | K10 max/rms %.2e %.2e | rms ratio %.2f" % (e_split + e_f32 + (ratio,)))
    assert e_split[0] < 2e-5, (tag, e_split)
    assert ratio <= 2.0, (tag, ratio)


# ------------------------------------------------------------------------------------------------ CPU emulation
def u_f64(w, scale):
    U = torch.einsum("ij,ocjk,lk->ocil", G, w.double(), G)
    return U * scale.double().view(-1, 1, 1, 1) if scale is not None else U


def pack_f16x2_emu(w, scale):
    """(hi, lo) fp16 images (cout, cin, 4, 4) and the epilogue factor (cout) as occd_wino_pack_weights_f16x2 defines them."""
    U = u_f64(w, scale)
    m = U.abs().amax(dim=(1, 2, 3))
    e = torch.frexp(m)[1]                                             # m in [2^(e-1), 2^e)
    k = torch.where(m > 0, (14 - e).clamp(-100, 100), torch.zeros_like(e))
    Us = (U * torch.pow(2.0, k.double()).view(-1, 1, 1, 1)).float()
    hi = Us.half()
    lo = (Us - hi.float()).half()
    return hi, lo, torch.pow(2.0, -(k.double() + 1)).float()


def emulate(case, x, w, scale, shift, res, split):
    """K10 (split = False) / K10h (split = True) arithmetic in torch: float32 transforms, float32 accumulation."""
    B, cin, cout, H, W, act, with_res, res_first, _ = case
    He, We = (H + 1) // 2 * 2, (W + 1) // 2 * 2
    d = F.pad(x, (1, 1 + We - W, 1, 1 + He - H)).unfold(2, 4, 2).unfold(3, 4, 2)           # B, cin, th, tw, 4, 4
    th, tw = d.shape[2], d.shape[3]
    V = torch.einsum("ij,bcyxjk,lk->ilbyxc", Bt, d, Bt).reshape(16, B * th * tw, cin)       # fp32
    mm = lambda v, u: torch.bmm(v.float(), u.float().permute(2, 3, 1, 0).reshape(16, cin, cout))
    if split:
        hi, lo, fac = pack_f16x2_emu(w, scale)
        us = (hi.float() / 2048.0).half()
        Vs = V * STAGE
        vh = Vs.half()
        vl = ((Vs - vh.float()) * 2048.0).half()
        M = (mm(vh, lo) + mm(vl, us) + mm(vh, hi)).double()
    else:
        M = mm(V, u_f64(w, scale).float()).double()
        fac = torch.ones(cout)
    M = M.view(4, 4, B, th, tw, cout)
    Y = torch.einsum("ij,jkbyxo,lk->boyixl", At, M, At).reshape(B, cout, th * 2, tw * 2)[:, :, :H, :W]
    y = (Y.float() * fac.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    if with_res and res_first:
        y = y + res
    y = ACT[act](y)
    if with_res and not res_first:
        y = y + res
    return y


@pytest.mark.parametrize("case", CASES)
def test_emulated_split_meets_the_gates_cpu(case):
    t = make(case)
    ref = reference(case, *t)
    check_gates(case, errors(emulate(case, *t, split=True), ref), errors(emulate(case, *t, split=False), ref))


@pytest.mark.parametrize("rng", RANGES)
def test_emulated_split_ranges_cpu(rng):
    t = make(RANGE_GEOM, *rng)
    ref = reference(RANGE_GEOM, *t)
    check_gates(rng, errors(emulate(RANGE_GEOM, *t, split=True), ref), errors(emulate(RANGE_GEOM, *t, split=False), ref))


def check_unpacked(hi, lo, fac, w, scale):
    """hi + lo against 2^k G g G^T scale: 2^-21 relative per element, or half an fp16 subnormal quantum (2^-25 in the scaled
    units, where lo is subnormal: elements below 2^-17 of their channel's largest)."""
    U = u_f64(w, scale)
    k = -(torch.log2(fac.double()) + 1)
    assert torch.equal(k, k.round())
    Us = U * torch.pow(2.0, k).view(-1, 1, 1, 1)
    m = Us.abs().amax(dim=(1, 2, 3))
    assert bool(((m >= 2.0 ** 13) & (m < 2.0 ** 14)).all())
    err = (hi.double() + lo.double() - Us).abs()
    assert bool((err <= torch.maximum(Us.abs() * 2.0 ** -21, torch.tensor(2.0 ** -25, dtype=torch.float64))).all())


def test_pack_emulation_round_trip_cpu():
    _, w, scale, _, _ = make((1, 33, 70, 7, 5, None, False, False, 0), decades=6)
    check_unpacked(*pack_f16x2_emu(w, scale), w, scale)


# ------------------------------------------------------------------------------------------------ GPU
def run_gpu(case, t):
    from occdepth_amd import hip
    x, w, scale, shift, res = (v.cuda() if v is not None else None for v in t)
    cout, act, res_first, hint = case[2], case[5], case[7], case[8]
    ys = []
    for upk in (hip.wino_pack_weights_f16x2(w, scale), hip.wino_pack_weights(w, scale)):
        ys.append(hip.conv2d_3x3_fused(x, upk, cout, shift, act, 0.01, res, res_first=res_first, tile_hint=hint))
    return ys


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_split_kernel_meets_the_gates_gpu(case, hip_lib):
    t = make(case)
    ref = reference(case, *t)
    y_split, y_f32 = run_gpu(case, t)
    check_gates(case, errors(y_split, ref), errors(y_f32, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("rng", RANGES)
def test_split_kernel_ranges_gpu(rng, hip_lib):
    t = make(RANGE_GEOM, *rng)
    ref = reference(RANGE_GEOM, *t)
    y_split, y_f32 = run_gpu(RANGE_GEOM, t)
    check_gates(rng, errors(y_split, ref), errors(y_f32, ref))


@pytest.mark.gpu
def test_pack_layout_round_trip_gpu(hip_lib):
    from occdepth_amd import hip
    cout, cin = 70, 33
    _, w, scale, _, _ = make((1, cin, cout, 7, 5, None, False, False, 0), decades=6)
    upk = hip.wino_pack_weights_f16x2(w.cuda(), scale.cuda())
    nblk, chunks = (cout + 31) // 32, (cin + 15) // 16
    raw = upk.image.cpu()
    assert raw.numel() == hip_lib.occd_wino_packed_f16x2_bytes(cout, cin) == chunks * 32 * nblk * 1024 + nblk * 128
    halves = raw[:chunks * 32 * nblk * 1024].view(torch.float16).view(chunks, 16, 2, nblk, 2, 32, 8)   # [..][lane >> 5][lane & 31][j]
    fac = raw[chunks * 32 * nblk * 1024:].view(torch.float32)
    # -> [image][cout][cin][xi]: cout = 32 blk + (lane & 31), cin = 16 chunk + 8 (lane >> 5) + j
    img = halves.permute(2, 3, 5, 0, 4, 6, 1).reshape(2, nblk * 32, chunks * 16, 16)
    assert float(img[:, cout:].abs().max()) == 0.0 and float(img[:, :, cin:].abs().max()) == 0.0     # padding: exact zeros
    hi, lo = (img[i, :cout, :cin].reshape(cout, cin, 4, 4) for i in range(2))
    check_unpacked(hi, lo, fac[:cout], w, scale)


@pytest.mark.gpu
def test_overflow_threshold_and_non_finite_inputs_gpu(hip_lib):
    from occdepth_amd import hip
    case = (1, 24, 32, 12, 20, None, False, False, 0)
    x, w, scale, shift, _ = make(case)
    upk, upk32 = hip.wino_pack_weights_f16x2(w.cuda(), scale.cuda()), hip.wino_pack_weights(w.cuda(), scale.cuda())
    run = lambda xi, u=upk: hip.conv2d_3x3_fused(xi.cuda(), u, 32, shift.cuda()).cpu()
    # a whole channel just below the threshold: |V| reaches 4 |x| (staged 2 V = 65512 rounds to 65504): finite, in tolerance
    xa = x.clone()
    xa[0, 3] = OVERFLOW_AT - 1
    ya = run(xa)
    e = errors(ya, reference(case, xa, w, scale, shift, None))
    print("below the threshold", e)
    assert bool(torch.isfinite(ya).all()) and e[0] < 2e-5
    # the 2x2 pixels of tile (2, 3) at the threshold: 2 V = 65520 rounds to Inf in that tile's patch only (its neighbours see
    # at most two of the four pixels); non-finite outputs there, nowhere outside the 4x4 patches that contain the pixels
    xb = x.clone()
    xb[0, 3, 4:6, 6:8] = OVERFLOW_AT
    yb = run(xb)
    bad = ~torch.isfinite(yb)
    assert bool(bad[0, :, 4:6, 6:8].any())
    reach = torch.zeros_like(bad)
    reach[0, :, 2:8, 4:10] = True                         # tiles whose patch (rows 2 ty - 1 .. 2 ty + 2) holds one of the pixels
    assert not bool((bad & ~reach).any())
    refb = reference(case, xb, w, scale, shift, None)
    assert float((yb.double() - refb).abs()[~reach].max() / refb.abs().max()) < 2e-5
    # NaN / Inf activations: non-finite exactly where K10's outputs are
    for v in (float("nan"), float("inf")):
        xc = x.clone()
        xc[0, 5, 7, 9] = v
        assert torch.equal(torch.isfinite(run(xc)), torch.isfinite(run(xc, upk32)))
    # fp16-subnormal staged operands are kept: activations at 2^-21 stage |2 V| < 2^-17, below the smallest fp16 normal
    # 2^-14.  hi then carries >= 4 bits and lo' 11 more (error ~2^-16); flushed to zero, lo' alone would leave 2^-12.
    xd = x * 2.0 ** -21
    shift0 = torch.zeros_like(shift)
    yd = hip.conv2d_3x3_fused(xd.cuda(), upk, 32, shift0.cuda()).cpu()
    ed = errors(yd, reference(case, xd, w, scale, shift0, None))
    print("subnormal operands", ed)
    assert ed[0] < 2.0 ** -14
    # non-finite weights: the operands stay float32
    from occdepth_amd import fused
    wbad = w.clone()
    wbad[3, 2, 1, 1] = float("inf")
    assert isinstance(fused.wino_pack(wbad.cuda(), scale.cuda()), torch.Tensor)
    with pytest.raises(ValueError):
        hip.wino_pack_weights_f16x2(wbad.cuda(), scale.cuda())


@pytest.mark.gpu
def test_split_kernel_is_deterministic_and_ignores_garbage_outside_gpu(hip_lib):
    from occdepth_amd import hip
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 24, 9, 35, generator=g).cuda()
    w = (torch.randn(32, 24, 3, 3, generator=g) * 0.1).cuda()
    upk = hip.wino_pack_weights_f16x2(w)
    a = hip.conv2d_3x3_fused(x, upk, 32)
    assert torch.equal(a, hip.conv2d_3x3_fused(x, upk, 32))
    # the same image between two NaN images of one batch: the halo rows and the channels past Cin of an image are its
    # neighbours in memory, and none of them is read as image content
    big = torch.full((3, 24, 9, 35), float("nan"), device="cuda")
    big[1] = x[0]
    assert torch.equal(a[0], hip.conv2d_3x3_fused(big, upk, 32)[1])
    ref = F.conv2d(x.double(), w.double(), padding=1)
    assert float((a.double() - ref).abs().max() / ref.abs().max()) < 2e-5


@pytest.fixture
def split_everywhere(monkeypatch):
    """The split on, and every geometry on K10h (the selection rule keeps launches it does not win on K10)."""
    from occdepth_amd import fused, hip
    saved = fused.WINO_SPLIT
    fused.set_wino_split("f16x2")
    monkeypatch.setattr(hip, "wino_f16x2_wins", lambda *a: True)
    yield
    fused.set_wino_split(saved)


@pytest.mark.gpu
def test_switch_and_operand_cache_gpu(hip_lib, split_everywhere):
    from occdepth_amd import fused, hip
    torch.manual_seed(3)
    conv, bn = torch.nn.Conv2d(24, 40, 3, padding=1, bias=False).cuda(), torch.nn.BatchNorm2d(40).cuda().eval()
    bn.running_mean.normal_(0, 0.2)
    bn.running_var.uniform_(0.5, 1.5)
    owner = torch.nn.Module()
    x = torch.randn(2, 24, 13, 18, device="cuda")
    upk, shift = fused.wino_fused_operands(owner, conv, bn)
    assert isinstance(upk, hip.WinoF16x2) and upk.f32 is not None
    y_split = hip.conv2d_3x3_fused(x, upk, 40, shift, "relu")
    fused.set_wino_split("fp32")
    upk32, shift32 = fused.wino_fused_operands(owner, conv, bn)            # the switch is part of the cache key
    assert isinstance(upk32, torch.Tensor)
    scale, _ = fused.bn_affine_cached(bn)
    y32 = hip.conv2d_3x3_fused(x, upk32, 40, shift32, "relu")
    assert torch.equal(y32, hip.conv2d_3x3_fused(x, hip.wino_pack_weights(conv.weight, scale), 40, shift, "relu"))
    assert not torch.equal(y32, y_split) and float((y32 - y_split).abs().max() / y32.abs().max()) < 2e-5
    fused.set_wino_split("f16x2")
    assert isinstance(fused.wino_fused_operands(owner, conv, bn)[0], hip.WinoF16x2)
    with pytest.raises(ValueError):
        fused.set_wino_split("bf16")


def _randomise_bn(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.normal_(0, 0.2)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.normal_(0, 0.2)


@pytest.mark.gpu
def test_upsample_level_with_the_split_gpu(hip_lib, split_everywhere):
    from occdepth_amd import hip
    from occdepth_amd.models.unet2d import UpSampleBN
    B, cup, cs, cout, h, w, H, W = (2, 40, 9, 16, 7, 9, 13, 18)
    torch.manual_seed(cup + cout)
    m = UpSampleBN(cup + cs, cout)
    _randomise_bn(m)
    m.eval()
    x, skip = torch.randn(B, cup, h, w), torch.randn(B, cs, H, W)
    saved = UpSampleBN.FUSED_MIN_PIXELS
    try:
        with torch.no_grad():
            ref = copy.deepcopy(m).double()(x.double(), skip.double())
            UpSampleBN.FUSED_MIN_PIXELS = 0
            with hip.profile() as prof:
                got = m.cuda()(x.cuda(), skip.cuda()).double().cpu()
    finally:
        UpSampleBN.FUSED_MIN_PIXELS = saved
    tags = {t.split(":")[0] for t in prof.rows}
    assert "wino_conv3x3_f16x2" in tags and "wino_conv3x3" not in tags, tags      # both convolutions of the level on K10h
    err = float((got - ref).abs().max() / ref.abs().max())
    print("UpSampleBN", f"{err:.2e}")
    assert got.shape == ref.shape and err < 3e-5


@pytest.mark.gpu
def test_basic_block_with_the_split_gpu(hip_lib, split_everywhere):
    from occdepth_amd import hip
    from occdepth_amd.models.flosp_depth.flosp_depth import BasicBlock
    torch.manual_seed(11)
    m = BasicBlock(24, 24)
    _randomise_bn(m)
    m.eval()
    x = torch.randn(2, 24, 13, 18)
    with torch.no_grad():
        ref = copy.deepcopy(m).double()(x.double())
        with hip.profile() as prof:
            got = m.cuda()(x.cuda()).double().cpu()
    tags = {t.split(":")[0] for t in prof.rows}
    assert "wino_conv3x3_f16x2" in tags and "wino_conv3x3" not in tags, tags
    err = float((got - ref).abs().max() / ref.abs().max())
    print("BasicBlock", f"{err:.2e}")
    assert got.shape == ref.shape and err < 3e-5


@pytest.mark.gpu
def test_selection_rule_by_workgroup_count_gpu(hip_lib):
    """An operand that carries both images (what fused.wino_pack builds) takes K10h on a launch of at least one workgroup
    (128 tiles x 32 couts) per CU and K10 below that; the profile tag tells which kernel ran."""
    from occdepth_amd import fused, hip
    saved = fused.WINO_SPLIT
    fused.set_wino_split("f16x2")
    try:
        torch.manual_seed(5)
        w = torch.randn(64, 16, 3, 3, device="cuda") * 0.1
        upk = fused.wino_pack(w)
        assert isinstance(upk, hip.WinoF16x2) and upk.f32 is not None
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        for (H, W), want in (((16, 32), "wino_conv3x3"), ((8, 32 * cus), "wino_conv3x3_f16x2")):
            x = torch.randn(1, 16, H, W, device="cuda")
            wgs = 2 * ((H // 2) * (W // 2) // 128)
            assert hip.wino_f16x2_wins(1, 16, 64, H, W) == (wgs >= cus) == (want == "wino_conv3x3_f16x2")
            with hip.profile() as prof:
                y = hip.conv2d_3x3_fused(x, upk, 64)
                torch.cuda.synchronize()
            assert {t.split(":")[0] for t in prof.rows} == {want}
            ref = F.conv2d(x.double(), w.double(), padding=1)
            assert float((y.double() - ref).abs().max() / ref.abs().max()) < 2e-5
    finally:
        fused.set_wino_split(saved)


def test_entry_point_argument_validation(hip_lib):
    """Host-side checks of the new entry points, as tests/test_abi.py has them for K10 (no launch for invalid arguments)."""
    import ctypes
    from occdepth_amd import hip
    assert hip_lib.occd_wino_packed_f16x2_bytes(80, 163) == 11 * 32 * 3 * 1024 + 3 * 128
    assert hip_lib.occd_wino_packed_f16x2_bytes(0, 8) < 0 and hip_lib.occd_wino_packed_f16x2_bytes(8, 0) < 0
    assert hip_lib.occd_wino_pack_weights_f16x2(None, None, None, 8, 8, None) == -1
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd(None, None) == -1
    a = hip.WinoArgs()
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd(ctypes.byref(a), None) == -1          # null pointers
    buf = (ctypes.c_float * 4)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    a.x = a.upk = a.y = ptr
    a.batch, a.cin, a.cout, a.H, a.W = 1, 8, 8, 0, 4
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd(ctypes.byref(a), None) == -1          # empty image
    a.H, a.act = 4, 7
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd(ctypes.byref(a), None) == -1          # act code
    a.act, a.cin, a.H, a.W = 0, 1 << 12, 1 << 10, 1 << 10
    assert hip_lib.occd_wino_conv3x3_f16x2_fwd(ctypes.byref(a), None) == -1          # 32-bit offsets inside one image


@pytest.mark.gpu
def test_pack_entry_point_refuses_non_finite_weights_gpu(hip_lib):
    """The C entry point itself returns the error (a caller without the Python wrapper must not get a garbage image)."""
    for bad in (float("inf"), float("nan")):
        w = torch.randn(40, 24, 3, 3, device="cuda")
        img = torch.empty(hip_lib.occd_wino_packed_f16x2_bytes(40, 24), dtype=torch.uint8, device="cuda")
        assert hip_lib.occd_wino_pack_weights_f16x2(w.data_ptr(), None, img.data_ptr(), 40, 24, None) == 0
        w[33, 5, 2, 0] = bad
        assert hip_lib.occd_wino_pack_weights_f16x2(w.data_ptr(), None, img.data_ptr(), 40, 24, None) == -1
    scale = torch.ones(40, device="cuda")
    scale[7] = float("inf")
    w = torch.randn(40, 24, 3, 3, device="cuda")
    assert hip_lib.occd_wino_pack_weights_f16x2(w.data_ptr(), scale.data_ptr(), img.data_ptr(), 40, 24, None) == -1
