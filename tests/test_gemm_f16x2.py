"""The two-term fp16 split ("f16x2") of the 2-D GEMMs that read pre-split weights (csrc/gemm_x3.hip): the weight image of
occd_gemm_f16x2_pack and the SPLIT = 2 forms of K16p (panel), K21 (panel split-K + reduce) and K16 on the A image.

CPU: a torch restatement of the scheme (row scaling, two-term split of both operands, the three products, float64
accumulation) against float64 next to torch's float32 matmul; the same restatement is the oracle of the pack image.
GPU: every route against float64 on the un-rounded operands beside the bf16x3 kernel on the same operands; range rows;
the non-finite / overflow contract; memory discipline; determinism; routing through the model's operand builders; the
config-2 golden frame under either setting of the switch."""
import pytest
import torch

DEV = "cuda"
F2X = 1                                                     # kF2XExp of csrc/device.h: activations are staged as 2^1 x


# ------------------------------------------------------------------------------------------------ the scheme in torch
def pack_rows(w):
    """(hi, lo, fac) of occd_gemm_f16x2_pack for a (M, K) float32 matrix: w' = 2^k[m] w with the row maximum in [2^13, 2^14)
    (an all-zero row: k = 0), hi = fp16(w'), lo = fp16(w' - hi), fac = 2^-(k + F2X)."""
    m = w.abs().amax(dim=1)
    e = torch.frexp(m)[1]                                   # m in [2^(e-1), 2^e)
    k = torch.where(m > 0, (14 - e).clamp(-100, 100), torch.zeros_like(e))
    ws = torch.ldexp(w, k.view(-1, 1).expand_as(w))         # exact
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return hi, lo, torch.ldexp(torch.ones_like(m), -(k + F2X))


def split_b(x):
    """x' = 2^F2X x = hi + 2^-11 lo' (split2_f16x8 / split2_f16x4 of csrc/device.h)."""
    xs = x * float(2 ** F2X)
    hi = xs.half()
    return hi, ((xs - hi.float()) * 2048.0).half()


def restated(w, x):
    """fac[m] * ((lo_a, hi_b) + (hs_a, lo'_b) + (hi_a, hi_b)) with every product and sum in float64."""
    hi, lo, fac = pack_rows(w)
    bh, bl = split_b(x)
    hs = (hi.float() * (1.0 / 2048.0)).half()               # fp16 product, denormals kept (v_pk_mul_f16)
    acc = lo.double() @ bh.double() + hs.double() @ bl.double() + hi.double() @ bh.double()
    return acc * fac.double().view(-1, 1)


CPU_SHAPES = [(256, 64, 100), (720, 1280, 231), (1440, 2560, 574), (2304, 384, 468), (384, 2304, 468)]


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restated_scheme_beats_float32_matmul(shape):
    """The scheme alone (no float32 accumulation): its error against float64 stays below torch's float32 matmul error on the
    same operands (measured 0.07 - 0.09e-6 of the output maximum against 0.3 - 0.95e-6)."""
    M, K, N = shape
    g = torch.Generator().manual_seed(M + K + N)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    x = torch.randn(K, N, generator=g) * 3.0
    ref = w.double() @ x.double()
    scale = ref.abs().max()
    err = float((restated(w, x) - ref).abs().max() / scale)
    err32 = float(((w @ x).double() - ref).abs().max() / scale)
    print(f"restated f16x2 {shape}: {err:.2e} (float32 matmul {err32:.2e}, ratio {err / err32:.2f})")
    assert err < err32, (shape, err, err32)


def test_pack_rows_scaling_rules():
    w = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, -3.0, 0.5, 0.0], [1e-20, 2e-20, 0.0, 0.0], [8192.0, 1.0, 2.0, 16383.0]])
    hi, lo, fac = pack_rows(w)
    assert float(fac[0]) == 0.5 and not hi[0].any() and not lo[0].any()              # all-zero row: k = 0
    top = (hi.float() + lo.float()).abs().amax(dim=1)[1:]
    assert bool(((top >= 2.0 ** 13) & (top < 2.0 ** 14)).all()), top
    back = (hi.double() + lo.double()) * fac.double().view(-1, 1) * 2.0 ** F2X
    assert float((back - w.double()).abs().max() / w.abs().max()) < 2.0 ** -21


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def hip():
    from occdepth_amd import hip as h
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU")
    h.load()
    return h


def _act(lin, act):
    return lin * torch.sigmoid(lin) if act == "swish" else lin


def _errs(got, ref):
    got = got.cpu().double()
    return float((got - ref).abs().max() / ref.abs().max()), float((got - ref).norm() / ref.norm())


def _gate(what, got, got3, lib, ref):
    """The two bounds of every accuracy case: max error below max(2e-6, 1.25 x the float32 library's) of the output maximum, rms
    error at most 1.5 x the bf16x3 kernel's on the same operands."""
    (e, r), (e3, r3), (el, _) = _errs(got, ref), _errs(got3, ref), _errs(lib, ref)
    print(f"gemm f16x2 {what}: max err {e:.2e} (bf16x3 {e3:.2e}, float32 library {el:.2e}), rms {r:.2e} (bf16x3 {r3:.2e})")
    assert got.shape == ref.shape
    assert e < max(2e-6, 1.25 * el), (what, e, el)
    assert r <= 1.5 * r3, (what, r, r3)


def _operands(batch, M, N, K, seed, xs=1.0, ws=1.0, row_scale=None):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(M, K, generator=g) / K ** 0.5 * ws
    if row_scale is not None:
        w = w * row_scale.view(-1, 1)
    x = torch.randn(batch, K, N, generator=g) * 3.0 * xs
    bias = torch.randn(M, generator=g) * float(w.abs().max() * K ** 0.5) * 3.0 * xs
    return w, x, bias


def _images(hip, w):
    wd = w.to(DEV)
    return wd, hip.GemmPacked(wd, "a", split="f16x2"), hip.GemmPacked(wd, "a")


def _lib(wd, xd, bd, act):
    return _act(torch.matmul(wd, xd) + bd.view(-1, 1), act)


def _panel_case(hip, batch, M, N, K, what, hint=8, **kw):
    w, x, bias = _operands(batch, M, N, K, M + N + K, **kw)
    ref = _act(torch.matmul(w.double(), x.double()) + bias.double().view(-1, 1), "swish")
    wd, ph, p3 = _images(hip, w)
    xd, bd = x.to(DEV), bias.to(DEV)
    with hip.profile() as prof:
        got = hip.gemm_x3(ph, xd, bias=bd, act="swish", tile_hint=hint)
    row = list(prof.rows)[0]
    assert row.endswith(" f16x2"), row
    got3 = hip.gemm_x3(p3, xd, bias=bd, act="swish", tile_hint=hint)
    _gate(what, got, got3, _lib(wd, xd, bd, "swish"), ref)
    return row


# K16p: (batch, M, N, K).  64-column panels (K <= 176): the K tail 32 + 16, a chip-filling launch, ragged M / N of every residue
# with a K tail of 8; 32-column panels (K > 176): a few-pixel launch, the two-step prefetch (K >= 512), the largest K that fits
PANEL_CASES = [(2, 288, 1848, 48), (2, 720, 3526, 160), (1, 77, 133, 72), (2, 77, 130, 72), (1, 77, 131, 72),
               (2, 576, 468, 384), (2, 320, 203, 640), (1, 256, 203, 848)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PANEL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_panel_accuracy(hip, case):
    row = _panel_case(hip, *case, what=f"K16p {case}")
    assert row.split(":")[0] == "gemm_f32x3_panel", row


SPLITK_CASES = [(1, 200, 131, 1000, (7, 9, 2)),             # K = 62.5 steps: the last chunk short and partial, two row ranges
                (2, 96, 70, 512, (2, 16, 3)),               # many 2-step chunks, N % 4 = 2, three row ranges
                (3, 40, 37, 256, (16, 1, 1)),               # ONE chunk
                (1, 200, 131, 1000, (16, 4, 1)),            # two-step prefetch, a short last chunk (15 steps)
                (2, 384, 468, 2304, None)]                  # the library's plan on the 1/32 stage's shape


@pytest.mark.gpu
@pytest.mark.parametrize("case", SPLITK_CASES, ids=lambda s: "x".join(map(str, s[:4])) + "_" + str(s[4]))
def test_splitk_accuracy_gate_skip_bias(hip, case):
    batch, M, N, K, plan = case
    g = torch.Generator().manual_seed(M + N + K)
    w = torch.randn(M, K, generator=g) / K ** 0.5
    y = torch.randn(batch, K, N, generator=g) * 2.0
    gate = torch.sigmoid(torch.randn(batch, K, generator=g))
    shift = torch.randn(M, generator=g)
    res = torch.randn(batch, M, N, generator=g)
    gated = y * gate.unsqueeze(-1)                           # float32 rounding of the product, as the reference's x * gate
    ref = torch.matmul(w.double(), gated.double()) + shift.double().view(-1, 1) + res.double()
    wd, ph, p3 = _images(hip, w)
    yd, gd, sd, rd = y.to(DEV), gate.to(DEV), shift.to(DEV), res.to(DEV)
    hip._SPLITK_WS.clear()
    with hip.profile() as prof:
        got = hip.gemm_x3_splitk(ph, yd, bias=sd, k_scale=gd, res=rd, plan=plan)
    row = [k for k in prof.rows if k.startswith("gemm_f32x3_splitk")]
    assert row and row[0].split(":")[0] == "gemm_f32x3_splitk" and row[0].endswith(" f16x2"), list(prof.rows)
    hip._SPLITK_WS[yd.device].fill_(float("nan"))            # stale workspace contents / pad columns must not matter
    again = hip.gemm_x3_splitk(ph, yd, bias=sd, k_scale=gd, res=rd, plan=plan)
    assert torch.equal(got, again)
    got3 = hip.gemm_x3_splitk(p3, yd, bias=sd, k_scale=gd, res=rd, plan=plan)
    lib = torch.matmul(wd, gated.to(DEV)) + sd.view(-1, 1) + rd
    _gate(f"K21 {case}", got, got3, lib, ref)
    # bias + swish, no gate / skip
    r2 = _act(torch.matmul(w.double(), y.double()) + shift.double().view(-1, 1), "swish")
    _gate(f"K21 swish {case}", hip.gemm_x3_splitk(ph, yd, bias=sd, act="swish", plan=plan),
          hip.gemm_x3_splitk(p3, yd, bias=sd, act="swish", plan=plan), _lib(wd, yd, sd, "swish"), r2)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [72, 392])
@pytest.mark.parametrize("hint", [1, 2, 3, 4, 5])
def test_prea_every_tile_variant(hip, hint, K):
    """K16 on the A image: every tile variant, K with 2 steps + a tail of 8 and 12 steps + a tail; gate + residual as well."""
    row = _panel_case(hip, 2, 512, 384, K, what=f"K16 preA hint {hint} K {K}", hint=hint)
    assert row.split(":")[0] == "gemm_f32x3_preA", row
    w, x, bias = _operands(2, 300, 333, K, hint + K)         # M, N tails in every variant
    g = torch.Generator().manual_seed(K)
    gate, res = torch.sigmoid(torch.randn(2, K, generator=g)), torch.randn(2, 300, 333, generator=g)
    gated = x * gate.unsqueeze(-1)
    ref = torch.matmul(w.double(), gated.double()) + bias.double().view(-1, 1) + res.double()
    wd, ph, p3 = _images(hip, w)
    kw = dict(bias=bias.to(DEV), k_scale=gate.to(DEV), res=res.to(DEV), tile_hint=hint)
    _gate(f"K16 preA gate+res hint {hint} K {K}", hip.gemm_x3(ph, x.to(DEV), **kw), hip.gemm_x3(p3, x.to(DEV), **kw),
          torch.matmul(wd, gated.to(DEV)) + bias.to(DEV).view(-1, 1) + res.to(DEV), ref)


@pytest.mark.gpu
def test_prea_hint0_long_k(hip):
    row = _panel_case(hip, 2, 720, 231, 1280, what="K16 preA hint 0 (2, 720, 231, 1280)", hint=0)
    assert row.split(":")[0] == "gemm_f32x3_preA", row


@pytest.mark.gpu
def test_pack_image_matches_the_restated_scheme(hip):
    """The image bit for bit: fragment order [row tile 32][k16][hi, lo][lane][8], zero padding, the factors behind it."""
    M, K = 77, 72
    w = _operands(1, M, 4, K, 5, row_scale=10.0 ** torch.linspace(-3, 3, M))[0]
    w[13] = 0.0
    ph = hip.GemmPacked(w.to(DEV), "a", split="f16x2")
    tiles, k16 = (M + 31) // 32, (K + 15) // 16
    assert ph.per == tiles * k16 * 1024 + tiles * 64 and ph.buf.dtype == torch.float16 and ph.buf.numel() == ph.per
    img = ph.buf[:tiles * k16 * 1024].cpu().view(tiles, k16, 2, 2, 32, 8)      # [rt][k16][term][k half][row][8]
    fac = ph.buf[tiles * k16 * 1024:].cpu().view(torch.float32)
    hi, lo, f = pack_rows(w)
    want = torch.zeros(2, tiles * 32, k16 * 16, dtype=torch.float16)
    want[0, :M, :K], want[1, :M, :K] = hi, lo
    want = want.view(2, tiles, 32, k16, 2, 8).permute(1, 3, 0, 4, 2, 5)
    assert torch.equal(img, want)
    assert torch.equal(fac[:M], f) and bool((fac[M:] == 0.5).all()) and float(fac[13]) == 0.5


RANGE_ROWS = [("x2^-16", dict(xs=2.0 ** -16)), ("x2^-8", dict(xs=2.0 ** -8)), ("x2^+8", dict(xs=2.0 ** 8)),
              ("w2^-12", dict(ws=2.0 ** -12)), ("w2^+6", dict(ws=2.0 ** 6)), ("row_scale", dict(row_scale=True))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", RANGE_ROWS, ids=[r[0] for r in RANGE_ROWS])
def test_range_rows(hip, name, kw):
    """Activations x 2^-16 / 2^-8 / 2^+8, weights x 2^-12 / 2^+6, a per-row weight scale spanning six decades: the same bounds,
    on K16p and on K16's A-image form."""
    M = 320
    if kw.get("row_scale"):
        kw = dict(row_scale=10.0 ** torch.linspace(-4, 2, M))
    _panel_case(hip, 2, M, 203, 264, what=f"range {name} K16p", **kw)
    _panel_case(hip, 2, M, 203, 264, what=f"range {name} K16 preA", hint=3, **kw)


@pytest.mark.gpu
def test_all_zero_weight_row_gives_act_of_bias_exactly(hip):
    w, x, bias = _operands(2, 96, 70, 512, 3)
    w[40] = 0.0
    ph, xd, bd = hip.GemmPacked(w.to(DEV), "a", split="f16x2"), x.to(DEV), bias.to(DEV)
    want = torch.empty(2, 70, device=DEV)
    for out in (hip.gemm_x3(ph, xd, bias=bd, tile_hint=8), hip.gemm_x3(ph, xd, bias=bd, tile_hint=4),
                hip.gemm_x3_splitk(ph, xd, bias=bd, plan=(8, 4, 1))):
        assert torch.equal(out[:, 40], want.fill_(float(bias[40])))


@pytest.mark.gpu
def test_non_finite_weight_is_refused_and_builder_keeps_bf16x3(hip):
    w = torch.randn(256, 64, device=DEV)
    for bad in (float("inf"), float("nan")):
        wb = w.clone()
        wb[200, 3] = bad
        with pytest.raises(ValueError):
            hip.GemmPacked(wb, "a", split="f16x2")
        gw = hip.GemmWeights(wb, "a", split="f16x2")
        assert hip.gemm_route(256, 100, 64, 2, a=gw).a == "f16x2" and gw.image("f16x2") is None      # refused, and remembered
        with hip.profile() as prof:
            hip.matmul(gw, torch.randn(2, 64, 100, device=DEV))
        launched = [k for k in prof.rows if "pack" not in k]
        assert len(launched) == 1 and "f16x2" not in launched[0] and launched[0].startswith("gemm_f32x3_panel"), prof.rows.keys()
        assert set(gw.images) == {"f16x2", "bf16x3"} and gw.images["bf16x3"].split == "bf16x3"
    assert hip.GemmWeights(w, "a", split="f16x2").image("f16x2").split == "f16x2"


@pytest.mark.gpu
def test_argument_rules(hip):
    w = torch.randn(256, 64, device=DEV)
    b = torch.randn(2, 64, 100, device=DEV)
    ph = hip.GemmPacked(w, "a", split="f16x2")
    with pytest.raises(RuntimeError):
        hip.GemmPacked(w, "b", split="f16x2")                # role "a" only
    for kw in (dict(sigmoid_a=True), dict(plain_bf16=True), dict(bias_n=torch.zeros(100, device=DEV)), dict(tile_hint=6),
               dict(tile_hint=7)):
        with pytest.raises(RuntimeError):
            hip.gemm_x3(ph, b, **kw)
    with pytest.raises(RuntimeError):                        # K16p's rules: no residual on hint 8
        hip.gemm_x3(ph, b, tile_hint=8, res=torch.zeros(2, 256, 100, device=DEV))
    with pytest.raises(RuntimeError):                        # K21's rules: chunks must tile K
        hip.gemm_x3_splitk(ph, b, plan=(8, 3, 1))
    assert hip.gemm_x3_supported(ph, b) and hip.gemm_x3(ph, b).shape == (2, 256, 100)


def _routes(hip, ph, xd, bd):
    yield "K16p", lambda **kw: hip.gemm_x3(ph, xd, bias=bd, act="swish", tile_hint=8, **kw)
    yield "K16 preA", lambda **kw: hip.gemm_x3(ph, xd, bias=bd, act="swish", tile_hint=1, **kw)
    yield "K21", lambda **kw: hip.gemm_x3_splitk(ph, xd, bias=bd, act="swish", plan=(5, 4, 2), **kw)


@pytest.mark.gpu
def test_nan_and_large_activations(hip):
    """A NaN activation reaches every output of its column and batch item and nothing else; 30000 is inside the operand range
    (|x| < 32760) and exact within the bound."""
    batch, M, N, K = 2, 300, 131, 312
    w, x, bias = _operands(batch, M, N, K, 11)
    wd, ph, p3 = _images(hip, w)
    bd = bias.to(DEV)
    xn = x.clone()
    xn[1, 100, 77] = float("nan")
    xl = x.clone()
    xl[0, 5, 9] = 30000.0
    ref = _act(torch.matmul(w.double(), xl.double()) + bias.double().view(-1, 1), "swish")
    for (what, run), (_, run_n), (_, run_l), (_, run_3) in zip(_routes(hip, ph, x.to(DEV), bd), _routes(hip, ph, xn.to(DEV), bd),
                                                                _routes(hip, ph, xl.to(DEV), bd), _routes(hip, p3, xl.to(DEV), bd)):
        clean, got = run(), run_n()
        bad = torch.zeros(batch, M, N, dtype=torch.bool, device=DEV)
        bad[1, :, 77] = True
        assert torch.equal(torch.isnan(got), bad), what
        assert torch.equal(got[~bad], clean[~bad]), what
        big = run_l()
        assert bool(torch.isfinite(big).all()), what
        _gate(f"{what} x = 30000", big, run_3(), _lib(wd, xl.to(DEV), bd, "swish"), ref)


@pytest.mark.gpu
def test_strided_views_inside_nan_frames(hip):
    """B and out are views inside NaN-filled frames, out on the padded_rows pitch: nothing outside the view is written and the
    padding is never read (a NaN read would poison a column)."""
    batch, M, N, K = 2, 300, 131, 312
    w, x, bias = _operands(batch, M, N, K, 13)
    wd, ph, _ = _images(hip, w)
    bd = bias.to(DEV)
    frame = torch.full((batch, K + 2, N + 7), float("nan"), device=DEV)
    frame[:, 1:1 + K, 3:3 + N] = x.to(DEV)
    xv = frame[:, 1:1 + K, 3:3 + N]
    for (what, run), (_, run_v) in zip(_routes(hip, ph, x.to(DEV), bd), _routes(hip, ph, xv, bd)):
        dense = run()
        assert hip.padded_rows((batch, M, N), DEV).stride(-2) == 160
        whole = torch.full((batch, M, 160), float("nan"), device=DEV)          # the padded_rows pitch, NaN in the pad columns
        out = whole[..., :N]
        if xv.device in hip._SPLITK_WS:
            hip._SPLITK_WS[xv.device].fill_(float("nan"))
        got = run_v(out=out)
        assert got.data_ptr() == out.data_ptr() and torch.equal(got, dense), what
        assert bool(torch.isnan(whole[..., N:]).all()), what


@pytest.mark.gpu
def test_determinism_and_graph_replay(hip):
    batch, M, N, K = 2, 300, 131, 312
    w, x, bias = _operands(batch, M, N, K, 17)
    ph = hip.GemmPacked(w.to(DEV), "a", split="f16x2")
    xd, bd = x.to(DEV), bias.to(DEV)
    for what, run in _routes(hip, ph, xd, bd):
        first = run().clone()
        assert torch.equal(first, run()), what
        out = torch.empty_like(first)
        run(out=out)                                         # (warm: workspace and LDS attributes exist before the capture)
        torch.cuda.synchronize()
        out.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run(out=out)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, first), what


# ------------------------------------------------------------------------------------------------ routing through the model
def _mbconv(hip):
    """One MBConv block's 1x1 convolutions at the smallest shapes the host rules take: expand 64 -> 768 on 2 x 6 x 6 pixels
    (K16p) and project 2304 -> 256 with gate and skip on 2 x 18 x 26 pixels (K21: the smallest launch of this shape family
    that hip.splitk_f16x2_wins gives to f16x2 -- 8 row tiles x 18 steps per workgroup)."""
    from occdepth_amd.models import efficientnet as en
    torch.manual_seed(0)
    owner = torch.nn.Module()
    conv_e, bn_e = torch.nn.Conv2d(64, 768, 1, bias=False), torch.nn.BatchNorm2d(768)
    conv_p, bn_p = torch.nn.Conv2d(2304, 256, 1, bias=False), torch.nn.BatchNorm2d(256)
    for m in (conv_e, bn_e, conv_p, bn_p):
        m.to(DEV).eval()
    x = torch.randn(2, 64, 6, 6, device=DEV)
    y2, skip = torch.randn(2, 2304, 18, 26, device=DEV), torch.randn(2, 256, 18, 26, device=DEV)
    gate = torch.sigmoid(torch.randn(2, 2304, device=DEV))
    assert hip.splitk_f16x2_wins(256, 468, 2304, 2)

    def block():
        return en.expand_gemm(owner, conv_e, bn_e, x, "swish"), en.project_conv(owner, conv_p, bn_p, y2, gate, skip)

    def explicit():
        sc, sh = en.bn_affine_cached(bn_e)
        we = (conv_e.weight.detach().float().flatten(1) * sc.view(-1, 1)).contiguous()
        y = hip.gemm_x3(hip.GemmPacked(we, "a"), x.view(2, 64, 36), bias=sh.contiguous(), act="swish").view(2, 768, 6, 6)
        sc, sh = en.bn_affine_cached(bn_p)
        wp = (conv_p.weight.detach().float().flatten(1) * sc.view(-1, 1)).contiguous()
        return y, hip.gemm_x3_splitk(hip.GemmPacked(wp, "a"), y2.view(2, 2304, 468), bias=sh.contiguous(), k_scale=gate,
                                     res=skip.view(2, 256, 468)).view(2, 256, 18, 26)
    return block, explicit


def _marked(prof, family):
    rows = [k for k in prof.rows if k.split(":")[0] == family]
    assert rows, (family, list(prof.rows))
    return [k.endswith(" f16x2") for k in rows]


@pytest.mark.gpu
def test_model_builders_follow_the_switch(hip):
    """Default f16x2: the rows of one MBConv block carry the marker; set_gemm_split('bf16x3'): bit-identical to explicit
    GemmPacked(w, 'a') launches, no marker; a flip mid-session takes effect at the next call."""
    from occdepth_amd import fused
    saved = fused.GEMM_SPLIT
    block, explicit = _mbconv(hip)
    try:
        hip.set_gemm_split("f16x2")
        with hip.profile() as prof:
            y_h, z_h = block()
        assert all(_marked(prof, "gemm_f32x3_panel")) and all(_marked(prof, "gemm_f32x3_splitk")), list(prof.rows)
        hip.set_gemm_split("bf16x3")
        assert hip.gemm_split() == "bf16x3"
        with hip.profile() as prof:
            y_3, z_3 = block()
        assert not any(_marked(prof, "gemm_f32x3_panel")) and not any(_marked(prof, "gemm_f32x3_splitk")), list(prof.rows)
        y_e, z_e = explicit()
        assert torch.equal(y_3, y_e) and torch.equal(z_3, z_e)
        assert not torch.equal(y_3, y_h) and float((y_3 - y_h).abs().max() / y_3.abs().max()) < 2e-6
        hip.set_gemm_split("f16x2")
        with hip.profile() as prof:
            y_b, z_b = block()
        assert all(_marked(prof, "gemm_f32x3_panel")) and torch.equal(y_b, y_h) and torch.equal(z_b, z_h)
        with pytest.raises(ValueError):
            hip.set_gemm_split("fp8")
    finally:
        fused.set_gemm_split(saved)


@pytest.mark.gpu
def test_splitk_host_rule_keeps_small_launches_on_bf16x3(hip):
    """hip.splitk_f16x2_wins on the seven K21 geometries of the config-2 frame: only 384 x 468 x 1344 (6 row tiles x 21 steps per
    workgroup, measured 1.00x) keeps bf16x3; project_conv follows it (no marker, bit-identical to the explicit bf16x3 launch)."""
    from occdepth_amd import fused
    from occdepth_amd.models import efficientnet as en
    frame = [(384, 468, 2304), (224, 1848, 1344), (160, 1848, 960), (640, 468, 3840), (640, 468, 2304), (224, 1848, 960),
             (384, 468, 1344)]
    assert [hip.splitk_f16x2_wins(M, N, K, 2) for M, N, K in frame] == [True] * 6 + [False]
    saved = fused.GEMM_SPLIT
    torch.manual_seed(2)
    owner, conv, bn = torch.nn.Module(), torch.nn.Conv2d(1344, 384, 1, bias=False).to(DEV).eval(), torch.nn.BatchNorm2d(384).to(DEV).eval()
    y, gate = torch.randn(2, 1344, 18, 26, device=DEV), torch.sigmoid(torch.randn(2, 1344, device=DEV))
    try:
        hip.set_gemm_split("f16x2")
        with hip.profile() as prof:
            got = en.project_conv(owner, conv, bn, y, gate, None)
        assert not any(_marked(prof, "gemm_f32x3_splitk")), list(prof.rows)
        sc, sh = en.bn_affine_cached(bn)
        wp = (conv.weight.detach().float().flatten(1) * sc.view(-1, 1)).contiguous()
        want = hip.gemm_x3_splitk(hip.GemmPacked(wp, "a"), y.view(2, 1344, 468), bias=sh.contiguous(), k_scale=gate)
        assert torch.equal(got.view(2, 384, 468), want)
    finally:
        fused.set_gemm_split(saved)


@pytest.mark.gpu
def test_decoder_up_block_follows_the_switch(hip):
    """One decoder level (UpSampleBN): its tap GEMM (288 rows, K = 32) takes K16p with the marker by default."""
    from occdepth_amd import fused
    from occdepth_amd.models.unet2d import UpSampleBN
    saved = fused.GEMM_SPLIT
    torch.manual_seed(1)
    up = UpSampleBN(skip_input=32 + 32, output_features=32).to(DEV).eval()
    x, skip = torch.randn(2, 32, 6, 8, device=DEV), torch.randn(2, 32, 12, 16, device=DEV)
    try:
        outs = {}
        for mode in ("f16x2", "bf16x3"):
            hip.set_gemm_split(mode)
            with torch.no_grad(), hip.profile() as prof:
                outs[mode] = up(x, skip)
            rows = [k for k in prof.rows if k.split(":")[0] in ("gemm_f32x3_panel", "gemm_f32x3_preA")]
            assert rows and all(k.endswith(" f16x2") == (mode == "f16x2") for k in rows), list(prof.rows)
        assert float((outs["f16x2"] - outs["bf16x3"]).abs().max() / outs["bf16x3"].abs().max()) < 1e-5
    finally:
        fused.set_gemm_split(saved)


@pytest.mark.gpu
def test_model_level_config2_golden(hip):
    """The config-2 golden frame (kitti_a100, eager) with OCCDEPTH_GEMM_SPLIT = f16x2 and = bf16x3: both within the golden bound
    (1e-3 of each output's maximum); the distance between the two settings and the largest |x| an f16x2 launch stages (operand
    limit 32760) are printed."""
    from test_parity_gpu import benched_batch, config2_errors
    from test_oracle_vs_golden import build_product
    from occdepth_amd import fused
    saved = fused.GEMM_SPLIT
    real, real_sk = hip.gemm_x3, hip.gemm_x3_splitk
    seen = []

    def spy(a, b, *args, **kw):
        if isinstance(a, hip.GemmPacked) and a.split == "f16x2":
            seen.append(float(b.abs().max()))
        return real(a, b, *args, **kw)

    def spy_sk(a, b, *args, **kw):
        if a.split == "f16x2":
            seen.append(float(b.abs().max()))
        return real_sk(a, b, *args, **kw)

    try:
        m, _, _ = build_product("kitti_a100")
        m = m.to(DEV).eval()
        batch = benched_batch()
        outs = {}
        for mode in ("f16x2", "bf16x3"):
            hip.set_gemm_split(mode)
            seen.clear()
            hip.gemm_x3, hip.gemm_x3_splitk = spy, spy_sk
            with torch.no_grad(), hip.profile() as prof:
                out = m(batch)
                torch.cuda.synchronize()
            hip.gemm_x3, hip.gemm_x3_splitk = real, real_sk
            marked = [k for k in prof.rows if k.endswith(" f16x2")]
            worst = config2_errors(out)
            print(f"config-2 golden, GEMM split {mode}: max rel {({k: f'{e:.2e}' for k, e in worst.items()})}, "
                  f"{len(marked)} f16x2 profile rows")
            if mode == "f16x2":
                print(f"f16x2 GEMM launches {len(seen)}, largest staged |x| {max(seen):.4g} (operand limit 32760)")
                assert marked and seen and max(seen) < 32760
            else:
                assert not marked and not seen
            assert max(worst.values()) < 1e-3, (mode, worst)
            outs[mode] = {k: v.float().clone() for k, v in out.items() if torch.is_tensor(v)}
        dist = {k: float((outs["f16x2"][k] - v).abs().max() / v.abs().max()) for k, v in outs["bf16x3"].items()}
        print(f"f16x2 against bf16x3, max |d| / max |bf16x3| per output: {({k: f'{e:.2e}' for k, e in dist.items()})}")
    finally:
        hip.gemm_x3, hip.gemm_x3_splitk = real, real_sk
        fused.set_gemm_split(saved)
