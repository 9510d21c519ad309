"""Depth-rendering loss (K36) on the GPU: csrc/render_loss.hip held to the float64 restatement of tests/test_render_loss.py
(walk, values, saturation, contention, determinism, capture, flip) and the model hook on the small KITTI configuration."""
import copy
import functools

import numpy as np
import pytest
import torch

from test_render_loss import B, C, CASES, STRIDES, R_CAM, Reference, case, rel_err, soft_logits

pytestmark = pytest.mark.gpu

LAYOUTS = ("planes", "rows")


def as_layout(logits, layout, requires_grad=False):
    """-> (the (B, C, X, Y, Z) tensor the loss reads, the leaf that receives the gradient).  "rows": the 3-D stack's
    channels-last voxel rows with a padded channel stride (8 floats for 5 classes)."""
    logits = logits.cuda()
    if layout == "planes":
        leaf = logits.clone().requires_grad_(requires_grad)
        return leaf, leaf
    rows = torch.zeros(logits.shape[:1] + logits.shape[2:] + (8,), device="cuda")
    rows[..., :logits.shape[1]] = logits.permute(0, 2, 3, 4, 1)
    rows.requires_grad_(requires_grad)
    return rows[..., :logits.shape[1]].permute(0, 4, 1, 2, 3), rows


def leaf_grad(leaf, layout, n_classes):
    g = leaf.grad
    if layout == "rows":
        assert not g[..., n_classes:].any()                      # the pad channels receive zeros
        g = g[..., :n_classes].permute(0, 4, 1, 2, 3)
    return g.cpu().numpy()


@functools.lru_cache(maxsize=None)
def expected(name, stride, offset, norm):
    """The restatement's (d^, opacity, L, #valid, d L / d logits) and the errors of the package's float32 torch formulation on
    the same inputs (CPU), computed once."""
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, ref = case(name)
    r_depth, r_alpha, _, _ = ref.images(stride, offset)
    r_loss, r_n = ref.loss(stride, offset, norm)
    r_grad = ref.grad_logits(stride, offset, norm)
    z = logits.clone().requires_grad_(True)
    loss, depth, alpha, n = rl.render_loss_torch(z, D, views, stride, offset, max_depth, norm)
    loss.backward()
    assert int(n) == r_n
    errs = dict(depth=rel_err(depth.detach().numpy(), r_depth), alpha=rel_err(alpha.detach().numpy(), r_alpha),
                loss=abs(float(loss.detach()) - r_loss) / abs(r_loss), grad=rel_err(z.grad.numpy(), r_grad))
    return dict(depth=r_depth, alpha=r_alpha, loss=r_loss, n=r_n, grad=r_grad), errs


# ------------------------------------------------------------------------------------------------------------ walk
@pytest.mark.parametrize("name", sorted(CASES))
def test_hard_logits_render_the_renderers_depth_bit_for_bit(name, hip_lib):
    """Logits of +-40 make a exactly 0 or 1 in float32: d^ is the depth occd_render_voxels reports where it hits and t_end
    where it does not, the rendered opacity is the hit mask -- at stride 1 and on the rows / columns of a strided pass."""
    from occdepth_amd import render
    from occdepth_amd.loss import render_loss as rl
    _, views, D, _, _ = case(name)
    dims, hw = CASES[name]["dims"], CASES[name]["image"]
    rng = np.random.default_rng(21)
    occ = rng.uniform(size=(B,) + dims) < 0.08
    z = np.zeros((B, C) + dims, dtype=np.float32)
    z[:, 0] = np.where(occ, -40.0, 40.0)
    labels = torch.from_numpy(occ.astype(np.uint8)).cuda()
    views = views.cuda()
    _, hit, _, depth = render.render_labels(labels, views[:, None], hw, return_aux=True, n_classes=2)
    hit, depth = hit[:, 0] >= 0, depth[:, 0]
    assert 0.05 < float(hit.float().mean()) < 0.95
    t_end = rl.slab_rays(views.cpu(), dims, hw)["t_end"].reshape(B, *hw).cuda()
    want = torch.where(hit, depth, t_end)
    for layout in LAYOUTS:
        logits, _ = as_layout(torch.from_numpy(z), layout)
        for stride, offset in STRIDES:
            d, a = rl.render_depth(logits, views, hw, stride=stride, offset=offset)
            sl = (slice(None), slice(offset[1], None, stride), slice(offset[0], None, stride))
            assert torch.equal(d, want[sl]), (layout, stride)
            assert torch.equal(a, hit[sl].float()), (layout, stride)


# ---------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("norm", ["abs", "rel"])
@pytest.mark.parametrize("stride,offset", STRIDES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_values_against_the_float64_restatement(name, layout, stride, offset, norm, hip_lib):
    """d^, opacity, L and d L / d logits as max|delta| / max|ref| against the restatement; allowance: twice the error of the
    package's float32 torch formulation on the same inputs plus 1e-6 (two float32 evaluations of the same sums in
    different orders).  #valid rays is exact."""
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, _ = case(name)
    ref, base = expected(name, stride, offset, norm)
    z, leaf = as_layout(logits, layout, requires_grad=True)
    fn = rl.RenderDepthLoss(stride=stride, max_depth=max_depth, norm=norm, offset=offset)
    loss = fn(z, D.cuda(), views.cuda())
    loss.backward()
    depth, alpha, n_valid = fn.last
    got = dict(depth=rel_err(depth.cpu().numpy(), ref["depth"]), alpha=rel_err(alpha.cpu().numpy(), ref["alpha"]),
               loss=abs(float(loss.detach()) - ref["loss"]) / abs(ref["loss"]),
               grad=rel_err(leaf_grad(leaf, layout, C), ref["grad"]))
    print("%s %s stride %d %s: " % (name, layout, stride, norm) +
          ", ".join("%s %.2e (torch f32 %.2e)" % (k, got[k], base[k]) for k in got))
    assert int(n_valid) == ref["n"]
    for k in got:
        assert got[k] <= 2.0 * base[k] + 1e-6, (k, got[k], base[k])


# ------------------------------------------------------------------------------------------------------ saturation
def test_saturated_and_empty_volumes(hip_lib):
    """A voxel whose p_0 underflows to 0 (a = 1 exactly) and an all-empty volume: finite gradients, d^ = t_end on the empty
    volume, H within its bound."""
    from occdepth_amd import hip
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, ref0 = case("small")
    dims, hw = CASES["small"]["dims"], CASES["small"]["image"]
    S = int(np.prod(dims))
    z = logits.clone()
    # every other one of the voxels the rays of frame 0 visit fourth (the camera sits inside: they all share the first)
    first = sorted({ref0.rays[0][v][u][3][3][0] for v in range(hw[0]) for u in range(hw[1]) if len(ref0.rays[0][v][u][3]) > 3})[::2]
    assert len(first) >= 3
    flat = z.reshape(B, C, S)
    flat[0, 0, first] = -120.0                                   # exp(-120) / sum underflows float32: p_0 = 0, a = 1
    flat[0, 1:, first] = 0.0
    z[1] = 0.0
    z[1, 0] = 120.0                                              # frame 1: all empty, a = 0 exactly
    ref = Reference(z.numpy(), views.numpy(), D.numpy(), max_depth, lambda b, v, u: ref0.rays[b][v][u])
    zg = z.cuda().requires_grad_(True)
    fn = rl.RenderDepthLoss(stride=1, max_depth=max_depth, norm="rel")
    loss = fn(zg, D.cuda(), views.cuda())
    opacity = hip.render_opacity(zg.detach())
    a = hip.render_opacity_decode(opacity)
    assert float(a[0, first[0]]) == 1.0 and not a[1].any()
    assert rel_err(a.cpu().numpy(), ref.a) <= 1e-6
    hsum = torch.zeros((B, S), dtype=torch.int64, device="cuda")
    hip.render_depth_bwd_rays(opacity, views.cuda(), dims, hw, 1, (0, 0), max_depth, D.cuda(), "rel", fn.last[0], hsum)
    assert int(hsum.abs().max()) < 1 << 62 and hsum[0].any()
    loss.backward()
    t_end = rl.slab_rays(views, dims, hw, max_depth=max_depth)["t_end"].reshape(B, *hw)
    assert torch.equal(fn.last[0][1].cpu(), t_end[1]) and not fn.last[1][1].any()
    g = zg.grad.cpu()
    assert torch.isfinite(g).all() and torch.isfinite(loss.detach())
    # a saturated voxel (p_0 = 0) gets a vanishing gradient, the empty frame none at all: a = 0 blocks every path
    assert not g.reshape(B, C, S)[0, :, first[0]].abs().max() > 1e-30 and not g[1].any()
    # values: the allowance of test_values_against_the_float64_restatement
    r_grad, r_loss = ref.grad_logits(1, (0, 0), "rel"), ref.loss(1, (0, 0), "rel")[0]
    zt = z.clone().requires_grad_(True)
    t_loss = rl.render_loss_torch(zt, D, views, 1, (0, 0), max_depth, "rel")[0]
    t_loss.backward()
    base = rel_err(zt.grad.numpy(), r_grad), abs(float(t_loss.detach()) - r_loss) / r_loss
    got = rel_err(g.numpy(), r_grad), abs(float(loss.detach()) - r_loss) / r_loss
    print("saturation: grad %.2e (torch f32 %.2e), loss %.2e (torch f32 %.2e)" % (got[0], base[0], got[1], base[1]))
    assert got[0] <= 2.0 * base[0] + 1e-6 and got[1] <= 2.0 * base[1] + 1e-6


# ------------------------------------------------------------------------------------------------------ contention
def test_every_ray_through_one_voxel(hip_lib):
    """A 64 x 64 image pressed against one voxel: all 4096 rays cross it first, 4096 integer atomics on one address (and on
    every voxel of the column under it): H equals the restatement's sums."""
    from occdepth_amd import hip
    dims, n = (6, 5, 7), 64
    X, Y, Z = dims
    S = X * Y * Z
    view = np.zeros(18, dtype=np.float32)
    view[:3] = [3.0, 2.0, Z + 0.5]
    view[3 + 1], view[6 + 0] = 1.0 / n, 1.0 / n                  # u spans voxel y = 2, v spans voxel x = 3
    view[9 + 2] = -1.0
    rng = np.random.default_rng(8)
    z = rng.standard_normal((1, 4) + dims).astype(np.float32)
    D = rng.uniform(0.6, Z - 0.1, (1, n, n)).astype(np.float32)
    max_depth = float(Z)                                         # the lowest voxel is entered at t = Z - 0.5 < max_depth
    ref = Reference(z, view[None], D, max_depth)
    column = [(3 * Y + 2) * Z + k for k in range(Z - 1, -1, -1)]
    assert all([s[0] for s in ref.rays[0][v][u][3]] == column for v in (0, 31, 63) for u in (0, 17, 63)) and ref.valid.all()
    zc = torch.from_numpy(z).cuda()
    views = torch.from_numpy(view)[None].cuda()
    opacity = hip.render_opacity(zc)
    depth, _, stats = hip.render_depth_fwd(opacity, views, dims, (n, n), gt_depth=torch.from_numpy(D).cuda())
    assert int(stats[1]) == n * n
    hsum = torch.zeros((1, S), dtype=torch.int64, device="cuda")
    hip.render_depth_bwd_rays(opacity, views, dims, (n, n), 1, (0, 0), max_depth, torch.from_numpy(D).cuda(), "abs", depth, hsum)
    got = hsum.cpu().numpy()[0] / 2.0 ** 32
    want = ref.grad_opacity() * (n * n) * (1.0 - ref.a)          # H_v = N dL/da_v (1 - a_v)
    assert not np.any(got[[i for i in range(S) if i not in column]])
    # every one of the N terms is a float32 evaluation of a few products and sums of quantities below t_max, on a d^ that
    # carries one rounding per step: (8 + 2 Z) 2^-24 t_max each, plus its Q32 rounding
    bound = n * n * ((8 + 2 * Z) * 2.0 ** -24 * (Z + 0.5) + 2.0 ** -32)
    err = np.abs(got - want[0]).max()
    print("contention: |H| max %.4g, error %.3g, bound %.3g" % (np.abs(want).max(), err, bound))
    assert np.abs(want[0][column]).max() > 1.0 and err <= bound


# ----------------------------------------------------------------------------------- determinism and self-cleaning
def test_two_runs_are_bit_equal_and_leave_h_clean(hip_lib):
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, _ = case("large")
    runs = []
    for _ in range(2):
        z = logits.cuda().requires_grad_(True)
        fn = rl.RenderDepthLoss(stride=1, max_depth=max_depth, norm="rel")
        loss = fn(z, D.cuda(), views.cuda())
        loss.backward()
        runs.append((loss.detach().clone(), z.grad.clone()))
        hsum = rl._hsum[(B, int(np.prod(logits.shape[2:])), str(z.device))]
        assert not hsum.any()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and runs[0][1].any()


# --------------------------------------------------------------------------------------------------------- capture
def test_captured_passes_replay_bit_equal_to_eager(hip_lib):
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, _ = case("small")
    fn = rl.RenderDepthLoss(stride=3, max_depth=max_depth, norm="abs", offset=(1, 2))
    inputs = []
    for seed in (0, 1, 2):
        rng = np.random.default_rng(100 + seed)
        inputs.append((torch.from_numpy(soft_logits(rng, B, C, CASES["small"]["dims"])).cuda(),
                       (D * float(rng.uniform(0.8, 1.2))).cuda()))

    def run(z, d):
        z = z.clone().requires_grad_(True)
        loss = fn(z, d, views.cuda())
        loss.backward()
        return loss.detach().clone(), z.grad.clone()

    eager = [run(z, d) for z, d in inputs]
    assert not torch.equal(eager[1][0], eager[2][0])
    sz = inputs[0][0].clone().requires_grad_(True)
    sd, sv = inputs[0][1].clone(), views.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(sz, sd, sv).backward()
        sz.grad = None
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss = fn(sz, sd, sv)
        s_loss.backward()
    for i in (1, 2):
        with torch.no_grad():
            sz.copy_(inputs[i][0])
            sd.copy_(inputs[i][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_loss.detach(), eager[i][0]) and torch.equal(sz.grad, eager[i][1]), i


# ------------------------------------------------------------------------------------------------------------ flip
def test_mirrored_depth_through_the_mirrored_view(hip_lib):
    """The loss of a mirrored D through the device-built mirrored view equals the loss of the unmirrored pair.  The camera is
    dyadic (focal 16, principal point W / 2, voxel 0.25 m), so the mirrored view's float32 rays ARE the plain view's rays of
    the mirrored columns and the two losses are the same sums: bit-equal."""
    from occdepth_amd.loss import render_loss as rl
    dims, hw, voxel = (16, 12, 8), (13, 22), 0.25
    k = torch.tensor([[16.0, 0.0, 11.0], [0.0, 16.0, 6.5], [0.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")[None].expand(2, 3, 3)
    E = torch.eye(4, dtype=torch.float64)
    E[:3, :3] = torch.from_numpy(R_CAM)
    E[:3, 3] = torch.from_numpy(-R_CAM @ np.array([0.375, 0.125, 0.0625]))
    E = E.cuda()[None].expand(2, 4, 4)
    origin = (0.0, -1.5, -1.0)
    rng = np.random.default_rng(31)
    z = torch.from_numpy(soft_logits(rng, 1, C, dims)).cuda().expand(2, C, *dims).contiguous()
    D = torch.from_numpy(rng.uniform(0.3, 3.5, (1, 1) + hw).astype(np.float32)).cuda()
    D = torch.where(torch.rand_like(D) < 0.2, torch.zeros_like(D), D)
    fn = rl.RenderDepthLoss(stride=1, max_depth=3.0, norm="rel")
    plain = rl.frame_views(k, E, origin, voxel, width=hw[1], flip=torch.tensor([False, False], device="cuda"))
    mixed = rl.frame_views(k, E, origin, voxel, width=hw[1], flip=torch.tensor([False, True], device="cuda"))
    assert torch.equal(plain[0], mixed[0]) and not torch.equal(plain[1], mixed[1])
    want = fn(z, torch.cat([D, D]), plain)
    d_plain = fn.last[0]
    got = fn(z, torch.cat([D, D.flip(-1)]), mixed)
    assert int(fn.last[2]) > 100 and torch.equal(fn.last[0][1].flip(-1), d_plain[1])
    assert torch.equal(got, want)


# ----------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def small(hip_lib):
    from test_train_step import _small_train_setup
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m, batch = _small_train_setup("kitti_small", "cuda")
    assert m.render_loss is None
    H, W = batch["img"].shape[-2:]
    g = torch.Generator().manual_seed(3)
    gt = (torch.rand((batch["img"].shape[0], 1, H, W), generator=g) * 20.0 + 1.0)
    gt = torch.where(torch.rand(gt.shape, generator=g) < 0.3, torch.zeros_like(gt), gt)
    return m.eval(), dict(batch, gt_depth=gt.cuda())


def test_step_adds_the_rendering_loss(small):
    from occdepth_amd.loss import render_loss as rl
    m0, batch = small
    off = copy.deepcopy(m0)
    off.step(batch, "train", None)
    keys_off, loss_off = sorted(off.logged), float(off.logged["train/loss"])
    assert "train/loss_render" not in keys_off
    m = copy.deepcopy(m0).enable_render_loss(weight=0.5, stride=2, max_depth=30.0)
    real, calls = m.render_loss["fn"], []

    class Spy(rl.RenderDepthLoss):
        def __call__(self, z, d, v):
            calls.append((z.detach().clone(), d.clone(), v.clone()))
            return super().__call__(z, d, v)

    real.__class__ = Spy
    m.step(batch, "train", None)
    assert sorted(m.logged) == sorted(keys_off + ["train/loss_render"])
    z, d, v = calls[0]
    assert len(calls) == 1 and int(real.last[2]) > 100           # the synthetic map gives the loss rays to work on
    alone = rl.RenderDepthLoss(stride=2, max_depth=30.0)(z, d, v) * 0.5
    assert torch.equal(alone, m.logged["train/loss_render"]) and float(alone) > 0
    # the other terms are what they are without the switch (the network runs a second time: 1e-6, as test_stereo_gpu)
    rest = float(m.logged["train/loss"]) - float(m.logged["train/loss_render"])
    assert abs(rest - loss_off) <= 1e-5 * abs(loss_off), (rest, loss_off)
    # val: the two image metrics as well; test: nothing
    m.step(batch, "val", None)
    assert {"val/loss_render", "val/render_abs_rel", "val/render_rmse"} <= set(m.logged)
    assert float(m.logged["val/render_rmse"]) > 0 and np.isfinite(float(m.logged["val/render_abs_rel"]))
    m.step(batch, "test", None)
    assert not any("render" in k for k in m.logged)
    m.step({k: t for k, t in batch.items() if k != "gt_depth"}, "train", None)
    assert "train/loss_render" not in m.logged


def test_rendering_loss_alone_reaches_the_parameters(small):
    m0, batch = small
    m = copy.deepcopy(m0).train().enable_render_loss(weight=1.0, stride=2, max_depth=30.0)
    m.zero_grad(set_to_none=True)
    m.logged = {}
    out = m(batch)
    loss = m._render_loss_step("train", batch, out["ssc_logit"], batch["gt_depth"])
    loss.backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert sum(float(g.abs().sum()) for g in grads) > 0


def test_captured_step_includes_the_rendering_loss(small):
    m0, batch = small
    first = batch
    second = dict(batch, gt_depth=(batch["gt_depth"] * 0.7).contiguous())
    eager = copy.deepcopy(m0).train().enable_render_loss(stride=2, max_depth=30.0)
    eager.step(second, "train", None)
    want = float(eager.logged["train/loss_render"])
    eager.step(first, "train", None)
    other = float(eager.logged["train/loss_render"])
    m = copy.deepcopy(m0).train().enable_fast_train()
    m.enable_render_loss(stride=2, max_depth=30.0)
    assert m._fast_train is None
    m._opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0, fused=True)      # the parameters stay put
    m.training_step(first, 0)                                   # captures (the warm-up runs on a snapshot), replays
    st = m._fast_train
    assert st["graph"] is not None and st["graph"].graph is not None, getattr(st["graph"], "error", None)
    got0 = float(m.logged["train/loss_render"])
    m.training_step(second, 1)                                  # copies the new depth map in, replays
    got1 = float(m.logged["train/loss_render"])
    print("loss_render: replayed %r / %r, eager %r / %r" % (got0, got1, other, want))
    assert abs(want - other) > 1e-3 * abs(want)                 # the two maps do give different losses
    # the bound of test_stereo_gpu's captured step: the backend may choose other convolution algorithms inside a capture
    assert abs(got0 - other) <= 1e-5 * abs(other) and abs(got1 - want) <= 1e-5 * abs(want)
