"""The Lovasz-softmax loss on the GPU (csrc/lovasz.hip on the K38 sort): the Jaccard increments against the closed-form
restatement exactly, loss and gradient against the float64 restatement within twice the error of the float32 torch
formulation, saturated and empty inputs, determinism, class chunks, capture, and the model hook."""
import copy

import numpy as np
import pytest
import torch

from test_lovasz import CLASSES, ONE_BITS, Q, closed_form, error_case, expected, logit_case

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
        assert not g[..., n_classes:].any()                      # the pad channels receive exact zeros
        g = g[..., :n_classes].permute(0, 4, 1, 2, 3)
    return g


def run(logits, target, layout="planes", class_chunk=None):
    from occdepth_amd.loss.lovasz_loss import LovaszSoftmaxLoss
    z, leaf = as_layout(logits, layout, True)
    fn = LovaszSoftmaxLoss(class_chunk=class_chunk)
    loss = fn(z, target.cuda())
    loss.backward()
    return loss.detach().clone(), leaf_grad(leaf, layout, logits.shape[1]).clone(), fn.last


# ------------------------------------------------------------------------------------------------- the exact seam
def sizes():
    from occdepth_amd import hip
    T = hip.SORT_TILE
    return [T - 1, T + 1, 3 * T + 17]


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("size", range(3))
def test_increments_equal_the_closed_form_exactly(size, C, kind, hip_lib):
    from occdepth_amd import hip
    from occdepth_amd.loss.lovasz_loss import lovasz_ref_from_errors
    N = sizes()[size]
    err, fg, valid = error_case(kind, C, N)
    assert not valid.all() and valid.any()                                        # holes
    want_q, want_lq, want_G = closed_form(err, fg, valid)
    q, lc, G, loss_q = hip.lovasz_from_errors(torch.from_numpy(err).cuda(), torch.from_numpy(fg).cuda(), torch.from_numpy(valid).cuda(), raw=True)
    assert np.array_equal(G.cpu().numpy(), want_G)
    assert np.array_equal(q.cpu().numpy(), want_q)                                # every element, sign and tie order included
    assert np.array_equal(loss_q.cpu().numpy(), want_lq)                          # the same integers
    # and the value against the definition (cumsum / Jaccard in the wide float), within the bound of the Q60 sum
    r_lc, _ = lovasz_ref_from_errors(err, fg.astype(bool), valid.astype(bool))
    bound = hip.lovasz_value_bound(N) + N * float(np.finfo(np.longdouble).eps)
    diff = np.abs(lc.cpu().numpy() - r_lc).max()
    print("N = %d C = %d %s: |L_c - ref| = %.3g, bound %.3g" % (N, C, kind, diff, bound))
    assert diff <= bound


# ------------------------------------------------------------------------------------------------- from the logits
@pytest.mark.parametrize("layout", LAYOUTS)
def test_loss_and_gradient_against_the_float64_restatement(layout, hip_lib):
    """The bar of K36: at most twice the error of the float32 torch formulation on the same inputs."""
    z, y = logit_case()
    ref, torch_err = expected()
    loss, grad, last = run(z, y, layout)
    e_loss = abs(float(loss) - ref["loss"])
    e_grad = np.abs(grad.cpu().numpy() - ref["grad"]).max() / np.abs(ref["grad"]).max()
    print("%s: loss error %.3g (torch float32 %.3g), gradient error %.3g (torch float32 %.3g)"
          % (layout, e_loss, torch_err["loss"], e_grad, torch_err["grad"]))
    assert ref["loss"] > 0.1 and (last[0] > 0).all()
    assert e_loss <= 2 * torch_err["loss"]
    assert e_grad <= 2 * torch_err["grad"]
    unknown = (y == 255)[:, None].expand_as(z).cuda()
    assert not grad[unknown].any() and grad[~unknown].any()


def test_saturated_logits_give_exact_errors(hip_lib):
    """Logits of +-40: every error is exactly 0 or 1 (or a tie of equal probabilities); the loss is finite and equals the
    restatement fed the kernel's own float32 errors, to the bound of the Q60 sum."""
    from occdepth_amd import hip
    from occdepth_amd.loss.lovasz_loss import lovasz_ref_from_errors
    z, y = logit_case("saturated")
    B, C = z.shape[:2]
    N = y.numel()
    keys = torch.empty((C, N), dtype=torch.int32, device="cuda")
    vals = torch.empty_like(keys)
    hip.lovasz_errors(z.cuda(), y.cuda(), 0, C, keys, vals)
    keys, vals = keys.cpu().numpy(), vals.cpu().numpy().view(np.uint32)
    valid = y.reshape(-1).numpy() != 255
    assert (keys[:, ~valid] == hip.LOVASZ_INVALID_KEY).all() and (keys[:, valid] <= ONE_BITS).all()
    err = (ONE_BITS - keys).astype(np.int32).view(np.float32)
    err[:, ~valid] = 0
    fg = (vals >> 31).astype(bool)
    assert np.array_equal(fg, (y.reshape(-1).numpy()[None] == np.arange(C)[:, None]) & valid[None])
    assert np.array_equal(vals & 0x7FFFFFFF, np.broadcast_to(np.arange(N, dtype=np.uint32), (C, N)))
    assert (err[:, valid] == 0).sum() > N // 4 and (err[:, valid] == 1).sum() > N // 4      # saturated: exact zeros and ones
    loss, grad, last = run(z, y)
    r_lc, _ = lovasz_ref_from_errors(err, fg, valid)
    lc = last[1].cpu().numpy() / 2.0 ** Q
    bound = hip.lovasz_value_bound(N) + N * float(np.finfo(np.longdouble).eps)
    print("saturated: |L_c - ref| = %.3g, bound %.3g" % (np.abs(lc - r_lc).max(), bound))
    assert np.isfinite(float(loss)) and torch.isfinite(grad).all()
    assert np.abs(lc - r_lc).max() <= bound
    assert abs(float(loss) - r_lc.mean()) <= 2.0 ** -24 * r_lc.mean() + bound          # one float32 rounding of the mean


def test_unknown_targets_and_absent_classes(hip_lib):
    z, y = logit_case()
    loss, grad, last = run(z, torch.full_like(y, 255))
    assert float(loss) == 0.0 and not grad.any() and not last[0].any() and not last[1].any()
    # classes 3 and 4 absent: #present is 3, their L_c is 0, and the loss is the mean over the three
    y3 = torch.where(y < 3, y, torch.full_like(y, 255))
    loss3, grad3, last3 = run(z, y3)
    lq = last3[1].cpu().numpy()
    assert (last3[0].cpu().numpy()[3:] == 0).all() and (lq[3:] == 0).all() and (lq[:3] > 0).all()
    want = np.float32(lq.astype(np.float64).sum() / (2.0 ** Q * 3.0))
    assert float(loss3) == float(want)
    # ... and the three present classes' values do not depend on how many classes the logits have beyond them being there:
    # the gradient of an absent class's column comes through the softmax only
    from occdepth_amd.loss.lovasz_loss import lovasz_ref
    r_loss, r_lc, r_grad = lovasz_ref(z.numpy(), y3.numpy())
    assert abs(float(loss3) - r_loss) <= 1e-6 and np.abs(grad3.cpu().numpy() - r_grad).max() <= 1e-6 * np.abs(r_grad).max() + 1e-9


def test_two_runs_and_class_chunks_are_bit_equal(hip_lib):
    z, y = logit_case()
    a, b = run(z, y), run(z, y)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].any()
    c = run(z, y, class_chunk=2)                                  # groups of 2, 2 and 1 classes over the same scratch
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert torch.equal(a[2][0], c[2][0]) and torch.equal(a[2][1], c[2][1])
    d = run(z, y, "rows", class_chunk=3)
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1])


def test_captured_loss_and_backward_replay_bit_equal_to_eager(hip_lib):
    from occdepth_amd.loss.lovasz_loss import LovaszSoftmaxLoss
    z0, y0 = logit_case()
    inputs = []
    for seed in (0, 1, 2):
        g = torch.Generator().manual_seed(200 + seed)
        y = torch.where(torch.rand(y0.shape, generator=g) < 0.2, torch.randint(0, CLASSES, y0.shape, generator=g).to(torch.uint8), y0)
        inputs.append(((z0 + 0.5 * torch.randn(z0.shape, generator=g)).cuda(), y.cuda()))
    fn = LovaszSoftmaxLoss()

    def eager_run(z, y):
        z = z.clone().requires_grad_(True)
        loss = fn(z, y)
        loss.backward()
        return loss.detach().clone(), z.grad.clone()

    eager = [eager_run(z, y) for z, y in inputs]
    assert not torch.equal(eager[1][0], eager[2][0])
    sz, sy = inputs[0][0].clone().requires_grad_(True), inputs[0][1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(sz, sy).backward()
        sz.grad = None
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss = fn(sz, sy)
        s_loss.backward()
    for i in (1, 2):
        with torch.no_grad():
            sz.copy_(inputs[i][0])
            sy.copy_(inputs[i][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_loss.detach(), eager[i][0]) and torch.equal(sz.grad, eager[i][1]), i


def test_targets_of_other_dtypes_run_on_the_kernels(hip_lib):
    from occdepth_amd.loss.lovasz_loss import LovaszSoftmaxLoss
    z, y = logit_case()
    fn = LovaszSoftmaxLoss()
    a = fn(z.cuda(), y.cuda())
    b = fn(z.cuda(), y.long())                                    # a CPU int64 target: moved and narrowed, same kernels
    assert fn.last is not None and torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def small(hip_lib):
    from test_train_step import _small_train_setup
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m, batch = _small_train_setup("kitti_small", "cuda")
    assert m.lovasz_loss is None
    return m.eval(), batch


def test_step_adds_the_lovasz_loss(small):
    from occdepth_amd.loss import lovasz_loss as ll
    m0, batch = small
    off = copy.deepcopy(m0)
    off.step(batch, "train", None)
    keys_off, loss_off = sorted(off.logged), float(off.logged["train/loss"])
    assert "train/loss_lovasz" not in keys_off
    m = copy.deepcopy(m0).enable_lovasz_loss(weight=0.5)
    real, calls = m.lovasz_loss["fn"], []

    class Spy(ll.LovaszSoftmaxLoss):
        def __call__(self, z, y):
            calls.append((z.detach().clone(), y.clone()))
            return super().__call__(z, y)

    real.__class__ = Spy
    m.step(batch, "train", None)
    assert sorted(m.logged) == sorted(keys_off + ["train/loss_lovasz"])
    z, y = calls[0]
    assert len(calls) == 1 and real.last is not None and int((real.last[0] > 0).sum()) >= 2      # on the kernels, classes present
    alone = ll.LovaszSoftmaxLoss()(z, y) * 0.5
    assert torch.equal(alone, m.logged["train/loss_lovasz"]) and float(alone) > 0
    # the total is the parent's total plus weight x the standalone loss (the network runs a second time: 1e-6, as
    # test_stereo_gpu and test_render_loss_gpu)
    rest = float(m.logged["train/loss"]) - float(m.logged["train/loss_lovasz"])
    assert abs(rest - loss_off) <= 1e-5 * abs(loss_off), (rest, loss_off)
    m.step(batch, "val", None)
    assert "val/loss_lovasz" in m.logged
    m.step(batch, "test", None)
    assert not any("lovasz" in k for k in m.logged)


def test_lovasz_loss_alone_reaches_the_parameters(small):
    m0, batch = small
    m = copy.deepcopy(m0).train().enable_lovasz_loss()
    m.zero_grad(set_to_none=True)
    out = m(batch)
    target, _ = m._step_labels(batch, out["ssc_logit"].device)
    m.lovasz_loss["fn"](out["ssc_logit"], target).backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert sum(float(g.abs().sum()) for g in grads) > 0


def test_captured_step_includes_the_lovasz_loss(small):
    m0, batch = small
    eager = copy.deepcopy(m0).train().enable_lovasz_loss()
    eager.step(batch, "train", None)
    want, want_total = float(eager.logged["train/loss_lovasz"]), float(eager.logged["train/loss"])
    m = copy.deepcopy(m0).train().enable_fast_train()
    m.enable_lovasz_loss()
    assert m._fast_train is None
    m._opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0, fused=True)      # the parameters stay put
    m.training_step(batch, 0)                                   # captures (the warm-up runs on a snapshot), replays
    st = m._fast_train
    assert st["graph"] is not None and st["graph"].graph is not None, getattr(st["graph"], "error", None)
    got0, total0 = float(m.logged["train/loss_lovasz"]), float(m.logged["train/loss"])
    m.training_step(batch, 1)
    got1 = float(m.logged["train/loss_lovasz"])
    print("loss_lovasz: replayed %r / %r, eager %r; total %r, eager %r" % (got0, got1, want, total0, want_total))
    # the bound of test_stereo_gpu's captured step: the backend may choose other convolution algorithms inside a capture
    assert want > 0 and abs(got0 - want) <= 1e-5 * want and abs(got1 - want) <= 1e-5 * want
    assert abs(total0 - want_total) <= 1e-5 * abs(want_total)
