"""GPU: the clip + AdamW kernels (csrc/optim.hip behind occdepth_amd/optim.py) against a float64 emulation, with torch's own
float32 path -- `clip_grad_norm_` + `AdamW(fused=True, capturable=True)` -- as the yardstick, and the clipped training step
captured into a hipGraph / driven in Lightning's order."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.05
SIZES = [1, 7, 4097, (1 << 20) + 3, 3_000_000]


def _tensors(seed=0):
    """Parameters of 1 .. a few million elements.  [0..4] own allocations; [5], [6] views at odd float offsets of one flat
    buffer (parameter misaligned, moments aligned: dword path); [7] aligned parameter whose GRADIENT is a view at an odd
    offset (what shard.GradBuckets attaches); [8] parameter, gradient and pre-set moments all views at the SAME odd offset
    (128-bit path behind a scalar head); [9] never gets a gradient."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda n: 0.1 * torch.randn(n, device="cuda", generator=g)
    ps = [torch.nn.Parameter(rnd(n)) for n in SIZES]
    flat = rnd(1 + 5001 + 2 + 70001)
    ps.append(torch.nn.Parameter(flat[1:1 + 5001]))
    ps.append(torch.nn.Parameter(flat[5004:5004 + 70001]))
    ps.append(torch.nn.Parameter(rnd(20001)))
    ps.append(torch.nn.Parameter(rnd(3 + 40007)[3:]))
    ps.append(torch.nn.Parameter(rnd(1000)))
    return ps


def _grads(ps, step, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + 17 + step)
    for i, p in enumerate(ps):
        if i == 9:
            p.grad = None
        elif i in (7, 8):
            off = 1 if i == 7 else 3
            buf = scale * torch.randn(off + p.numel(), device="cuda", generator=g)
            p.grad = buf[off:]
        else:
            p.grad = scale * torch.randn(p.shape, device="cuda", generator=g)


def _optimizer(ps, lr):
    from occdepth_amd import train_graph
    opt = train_graph.make_capturable(torch.optim.AdamW(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=WD, fused=True))
    p = ps[8]                                               # moments as views at the parameter's own odd offset
    opt.state[p] = {"step": torch.zeros((), dtype=torch.float32, device="cuda"),
                    "exp_avg": torch.zeros(3 + p.numel(), device="cuda")[3:],
                    "exp_avg_sq": torch.zeros(3 + p.numel(), device="cuda")[3:]}
    return opt


class _Float64:
    """clip_grad_norm_ + AdamW in float64 (the formulas of torch/nn/utils/clip_grad.py and torch/optim/adamw.py)."""

    def __init__(self, ps):
        self.p = [p.detach().double() for p in ps]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(ps)

    def step(self, ps, lr, max_norm):
        gs = [None if p.grad is None else p.grad.detach().double() for p in ps]
        total = torch.sqrt(sum((g * g).sum() for g in gs if g is not None))
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
        for i, g in enumerate(gs):
            if g is None:
                continue
            g = g * coef
            self.t[i] += 1
            self.p[i] *= 1 - lr * WD
            self.m[i] += (1 - BETAS[0]) * (g - self.m[i])
            self.v[i] = BETAS[1] * self.v[i] + (1 - BETAS[1]) * g * g
            bc1, bc2 = 1 - BETAS[0] ** self.t[i], 1 - BETAS[1] ** self.t[i]
            self.p[i] -= (lr / bc1) * self.m[i] / (self.v[i].sqrt() / bc2 ** 0.5 + EPS)
        return float(total)


def _run(which, max_norm, scale=1.0, steps=4):
    """4 steps, device lr changed between steps 2 and 3.  Returns per-step norms, the parameters and the optimizer."""
    from occdepth_amd import optim
    ps = _tensors()
    opt = _optimizer(ps, 1e-3)
    ref = _Float64(ps) if which == "float64" else None
    norms = []
    for step in range(steps):
        if step == 2:
            opt.param_groups[0]["lr"].fill_(4e-4)
        _grads(ps, step, scale)
        if which == "float64":
            norms.append(ref.step(ps, float(opt.param_groups[0]["lr"]), max_norm))
        elif which == "torch":
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
            opt.step()
        else:
            keep = [None if p.grad is None else p.grad.clone() for p in ps]
            norms.append(float(optim.clip_adamw_step(opt, max_norm)))
            assert all(k is None or torch.equal(k, p.grad) for k, p in zip(keep, ps)), "p.grad must stay unscaled"
    return norms, (ref.p if ref else [p.detach().double() for p in ps]), opt, ps


@pytest.mark.parametrize("setting", ["inactive", "active", "tiny"])
def test_kernels_against_float64_with_torch_as_yardstick(setting, hip_lib):
    """Error bound: the kernels' error against the float64 emulation is at most 2x that of torch's float32 path on the same
    inputs, for total_norm (largest error over the 4 steps) and for the final parameters (largest absolute error over all
    tensors).  The `step` counters equal torch's exactly; the gradient-less parameter gets no state in either."""
    n64 = _run("float64", 1e30)[0][0]
    max_norm = {"inactive": 4.0 * n64, "active": 0.5 * n64, "tiny": 1e-3}[setting]
    norm64, p64, _, _ = _run("float64", max_norm)
    norm_t, p_t, opt_t, ps_t = _run("torch", max_norm)
    norm_k, p_k, opt_k, ps_k = _run("kernels", max_norm)
    err = lambda a, b: max(float((x - y).abs().max()) for x, y in zip(a, b))
    e_norm_t = max(abs(a - b) for a, b in zip(norm_t, norm64))
    e_norm_k = max(abs(a - b) for a, b in zip(norm_k, norm64))
    e_p_t, e_p_k = err(p_t, p64), err(p_k, p64)
    print(f"{setting}: total_norm {norm64[0]:.6f} max_norm {max_norm:.6g}; |total_norm - f64| torch {e_norm_t:.3e} kernels "
          f"{e_norm_k:.3e}; max |p - f64| torch {e_p_t:.3e} kernels {e_p_k:.3e}")
    assert e_norm_k <= 2.0 * e_norm_t, (e_norm_k, e_norm_t)
    assert e_p_k <= 2.0 * e_p_t, (e_p_k, e_p_t)
    for i, (a, b) in enumerate(zip(ps_k, ps_t)):
        if i == 9:
            assert len(opt_k.state[a]) == 0 and len(opt_t.state[b]) == 0 and torch.equal(a, b)
            continue
        assert torch.equal(opt_k.state[a]["step"], opt_t.state[b]["step"]) and float(opt_k.state[a]["step"]) == 4.0, i
        for k in ("exp_avg", "exp_avg_sq"):
            x, y = opt_k.state[a][k], opt_t.state[b][k]
            assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max()) + 1e-30, (i, k)
    # a later plain torch step on the kernels' state keeps working
    _grads(ps_k, 4)
    opt_k.step()
    assert float(opt_k.state[ps_k[0]]["step"]) == 5.0


def test_two_runs_are_bit_identical(hip_lib):
    from occdepth_amd import optim
    a, b = _run("kernels", 3.0), _run("kernels", 3.0)
    assert a[0] == b[0]
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    for p, q in zip(a[3], b[3]):
        for k, v in a[2].state[p].items():
            assert torch.equal(v, b[2].state[q][k]), k
    # the norm pass alone: same bits again, and nothing else moves
    before = [p.detach().clone() for p in a[3]]
    n1, n2 = optim.grad_norm(a[2]), optim.grad_norm(a[2])
    assert torch.equal(n1, n2) and float(n1) == a[0][-1]
    assert all(torch.equal(x, y) for x, y in zip(before, a[3])) and float(a[2].state[a[3][0]]["step"]) == 4.0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_gives_torchs_pattern(bad, hip_lib):
    """One Inf element: total_norm Inf, clip_coef 0, that element's product NaN -> exactly one parameter element NaN.
    One NaN element: total_norm and clip_coef NaN -> every stepped parameter NaN.  Same pattern as the torch sequence."""
    from occdepth_amd import optim, train_graph
    out = {}
    for which in ("torch", "kernels"):
        g = torch.Generator(device="cuda").manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(n, device="cuda", generator=g)) for n in (5, 300, 9000)]
        opt = train_graph.make_capturable(torch.optim.AdamW(ps, lr=1e-3, weight_decay=WD, fused=True))
        for step in range(2):
            for p in ps:
                p.grad = torch.randn(p.shape, device="cuda", generator=g)
            if step == 1:
                ps[1].grad[17] = bad
            if which == "torch":
                norm = torch.nn.utils.clip_grad_norm_(ps, 1.0)
                opt.step()
            else:
                norm = optim.clip_adamw_step(opt, 1.0)
        out[which] = (float(norm), [torch.isfinite(p.detach()).cpu() for p in ps], [torch.isnan(p.detach()).cpu() for p in ps])
    (nt, ft, at), (nk, fk, ak) = out["torch"], out["kernels"]
    assert (nt == nk) or (nt != nt and nk != nk), (nt, nk)
    assert all(torch.equal(x, y) for x, y in zip(ft, fk)) and all(torch.equal(x, y) for x, y in zip(at, ak))
    n_bad = sum(int((~f).sum()) for f in fk)
    assert n_bad == (1 if bad == float("inf") else 5 + 300 + 9000)


# ------------------------------------------------------------------------------------------------ the training step
def _first_norm(m0, batch):
    from occdepth_amd import train_graph
    m = copy.deepcopy(m0).train()
    m.cur_batch = 0
    opt = train_graph.make_capturable(torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True))
    opt.zero_grad(set_to_none=True)
    m.training_step(batch, 0).backward()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    return float(torch.linalg.vector_norm(torch.stack([g.norm() for g in grads]))), sum(g.numel() for g in grads)


EPS_OVER_RMS = 10.0          # see test_captured_clipped_step_matches_eager_clip_grad_norm_gpu
LR = 1e-4 * EPS_OVER_RMS


def test_captured_clipped_step_matches_eager_clip_grad_norm_gpu(hip_lib):
    """GraphedTrainStep(grad_clip=c), c = half the norm of the first eager step (clipping certainly active), on the reduced
    SemanticKITTI model in training mode.  Capturing trains nothing; four replays match four eager steps that use
    clip_grad_norm_ + opt.step() within the bounds of test_train_step.py::test_whole_step_hipgraph_matches_eager_gpu (1e-5 on
    the first loss, 1.5e-2 on later losses, 5e-3 on the parameter); an unclipped captured run differs from the clipped one
    by MORE than those bounds, so the comparison can tell; `model.logged["train/grad_norm"]` after a replay is the norm
    of the gradients that replay left in `p.grad` (unscaled), within the kernel test's bound: its error against float64 at
    most 2x that of torch's float32 total norm of the same gradients.

    Optimizer settings.  AdamW's update m / (sqrt(v) + eps) does not change when every gradient is scaled by the same
    factor, so with the default eps = 1e-8 a clip whose coefficient stays near 0.5 is invisible in losses and parameters
    (measured with lr 1e-4: clipped vs unclipped 1.8e-3 on the loss, less than the 4e-3 by which two identical captured runs
    differ).  To see the clip, the update must depend on the gradient's scale: eps = 10 x the rms gradient element of the
    first step (taken from the same eager backward that gives c), where the update is close to lr g / eps, and lr = 10 x
    1e-4 so that an element with the rms gradient still moves by about 1e-4 per step, as in the test the bounds come from.
    Measured on MI355X with these settings: eager vs captured 2.3e-3 on the losses and 6e-5 on the parameter, two
    identical captured runs 5e-3, clipped vs unclipped 1.3e-2, 1.7e-2, 3.0e-2 on losses 1..3."""
    from test_train_step import _small_train_setup
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, batch = _small_train_setup("kitti_small", "cuda")
    norm, n_elems = _first_norm(m0, batch)
    c, eps = 0.5 * norm, EPS_OVER_RMS * norm / n_elems ** 0.5
    assert c > 0
    runs = _clip_runs(m0, batch, c, ("eager_clip", "graph_clip", "graph_noclip"), LR, eps)
    (le, pe, ne), (lg, pg, ng), (lu, pu, _) = runs["eager_clip"], runs["graph_clip"], runs["graph_noclip"]
    print("clip", c, "eps", eps, "eager", le, ne, "graph", lg, ng, "unclipped graph", lu)
    print("eager vs graph: losses", [abs(a - b) / abs(a) for a, b in zip(le, lg)], "parameter",
          float((pe - pg).abs().max() / pe.abs().max()))
    print("clipped vs unclipped: losses", [abs(a - b) / abs(a) for a, b in zip(lg, lu)], "parameter",
          float((pg - pu).abs().max() / pg.abs().max()))
    assert ne[0] > c and ng[0] > c
    assert abs(le[0] - lg[0]) <= 1e-5 * abs(le[0]), (le, lg)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(le, lg)), (le, lg)
    assert float((pe - pg).abs().max() / pe.abs().max()) < 5e-3
    assert any(abs(a - b) > 1.5e-2 * abs(a) for a, b in zip(lg, lu)) or float((pg - pu).abs().max() / pg.abs().max()) >= 5e-3, (lg, lu)


def _clip_runs(m0, batch, c, modes, lr, eps):
    """Four steps of the reduced model from the same state: "eager_clip" = zero_grad, training_step, backward,
    clip_grad_norm_, opt.step(); "graph_clip" / "graph_noclip" = replays of GraphedTrainStep with / without grad_clip."""
    from occdepth_amd import train_graph
    runs = {}
    for mode in modes:
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        opt = train_graph.make_capturable(torch.optim.AdamW(m.parameters(), lr=lr, eps=eps, fused=True))
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.4)
        gs = train_graph.GraphedTrainStep(m, opt, batch, warmup=2, grad_clip=c if mode == "graph_clip" else None)
        if mode != "eager_clip":
            before = {k: v.detach().clone() for k, v in m.state_dict().items()}
            assert gs.capture(), gs.error
            after = m.state_dict()
            assert all(torch.equal(before[k], after[k]) for k in before), "capture must not train"
            assert m.cur_batch == 0 and m.train_metrics.count == 1e-8
            assert all(float(v.abs().max()) == 0.0 for st in opt.state.values() for v in st.values() if torch.is_tensor(v))
            assert m.train_metrics.hist is None or int(m.train_metrics.hist.sum()) == 0
        losses, norms = [], []
        for i in range(4):
            if mode == "eager_clip":
                opt.zero_grad(set_to_none=True)
                loss = m.training_step(batch, 0)
                loss.backward()
                norms.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), c)))
                opt.step()
                losses.append(float(loss))
            else:
                losses.append(float(gs()))
                if mode == "graph_clip":
                    norms.append(float(m.logged["train/grad_norm"]))
                    grads = [p.grad for p in m.parameters() if p.grad is not None]
                    n64 = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads)))
                    n32 = float(torch.nn.utils.get_total_norm(grads))
                    print(f"replay {i}: logged norm {norms[-1]!r} float64 {n64!r} torch float32 {n32!r}")
                    assert abs(norms[-1] - n64) <= 2.0 * abs(n32 - n64), (norms[-1], n32, n64)
            sched.step()
        assert m.cur_batch == 4
        assert ("train/grad_norm" in m.logged) == (mode == "graph_clip")
        runs[mode] = (losses, next(iter(m.net_3d_decoder.parameters())).detach().float().cpu().clone(), norms)
    return runs


class ClipTrainer:
    """pytorch-lightning 1.4.9's loop for fit, with `Trainer(gradient_clip_val=...)`: under automatic optimisation the
    trainer clips between backward and optimizer.step (scripts/train.py:188,204); under manual optimisation it calls
    training_step alone and clips nothing -- the module reads `trainer.gradient_clip_val`."""

    def __init__(self, model, gradient_clip_val):
        self.model, self.gradient_clip_val, self.gradient_clip_algorithm = model, gradient_clip_val, "norm"
        self.logged = {}
        model.log = lambda key, value, **kw: self.logged.__setitem__(key, float(value))
        model.trainer = self

    def fit(self, batches):
        (opt,), _ = self.model.configure_optimizers()
        self.losses, self.norms = [], []
        self.model.on_train_epoch_start()
        for i, b in enumerate(batches):
            if getattr(self.model, "automatic_optimization", True):
                opt.zero_grad()
                loss = self.model.training_step(b, i)
                loss.backward()
                self.norms.append(float(torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.gradient_clip_val)))
                opt.step()
            else:
                loss = self.model.training_step(b, i)
                assert not loss.requires_grad
                self.norms.append(self.logged["train/grad_norm"])
            self.losses.append(float(loss.detach()))
            self.model.on_train_batch_end(None, b, i, 0)


def test_fast_train_reads_the_trainers_clip_value_gpu(hip_lib):
    """An unmodified scripts/train.py with OCCDEPTH_FAST_TRAIN=1: the module finds `gradient_clip_val` on its trainer and the
    fast path (captured step, three frames) trains like the same module under automatic optimisation with the trainer
    applying clip_grad_norm_, within the bounds of test_whole_step_hipgraph_matches_eager_gpu."""
    from test_lightning_hooks import _gpu_frames
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, frames = _gpu_frames("kitti_small", 3)
    c = 0.5 * _first_norm(m0, frames[0])[0]
    runs = {}
    for name in ("plain", "fast"):
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        if name == "fast":
            m.enable_fast_train()
        tr = ClipTrainer(m, c)
        tr.fit(frames)
        runs[name] = (tr.losses, next(iter(m.net_3d_decoder.parameters())).detach().float().cpu().clone(), tr.norms)
        if name == "fast":
            st = m._fast_train
            assert st["graph"] is not None and st["graph"].graph is not None, getattr(st["graph"], "error", None)
            assert st["graph"].grad_clip == c
    (lp, pp, np_), (lf, pf, nf) = runs["plain"], runs["fast"]
    print("plain", lp, np_, "fast", lf, nf)
    assert np_[0] > c
    assert abs(lp[0] - lf[0]) <= 1e-5 * abs(lp[0]), (lp, lf)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(lp, lf)), (lp, lf)
    assert float((pp - pf).abs().max() / pp.abs().max()) < 5e-3
    assert nf[0] > c                                        # the fast path clipped too (norms are printed above)
