"""GPU: gradient accumulation fused into clip + AdamW (occd_accum_clip_adamw in csrc/optim.hip behind optim.GradWindow)
against a float64 emulation with torch's float32 sequence -- `p.grad = g0 / n; p.grad += g1 / n; ...; clip_grad_norm_;
AdamW(fused=True, capturable=True)` -- as the yardstick; the same launches captured into a hipGraph; the accumulating
training step captured whole and driven in Lightning's order."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

BETAS, EPS, WD = (0.9, 0.999), 1e-8, 0.05
CHUNK = 8192
SIZES = [1, 7, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 5]
NO_GRAD = 9
GRAD_OFFSET = {7: 1, 8: 3}       # parameters whose gradient is a view at an odd float offset


def _tensors(seed=0):
    """The smallest shapes at which the kernels can go wrong (the chunk is 8192 elements).  [0..4] own allocations; [5], [6]
    views at odd float offsets of one flat buffer (parameter and accumulator misaligned, moments and gradient aligned);
    [7] aligned parameter whose GRADIENT is a view at an odd offset (what shard.GradBuckets attaches); [8] parameter,
    gradient and pre-set moments all views at the SAME odd offset (128-bit path behind a scalar head, over two chunks); [9]
    never gets a gradient."""
    from occdepth_amd import hip
    assert hip.OPTIM_CHUNK == CHUNK
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda n: 0.1 * torch.randn(n, device="cuda", generator=g)
    ps = [torch.nn.Parameter(rnd(n)) for n in SIZES]
    flat = rnd(1 + 5001 + 2 + 9001)
    ps.append(torch.nn.Parameter(flat[1:1 + 5001]))
    ps.append(torch.nn.Parameter(flat[5004:5004 + 9001]))
    ps.append(torch.nn.Parameter(rnd(CHUNK + 3)))
    ps.append(torch.nn.Parameter(rnd(3 + CHUNK + 5)[3:]))
    ps.append(torch.nn.Parameter(rnd(1000)))
    return ps


def _grad_values(ps, micro, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(17 + micro)
    out = []
    for i, p in enumerate(ps):
        if i == NO_GRAD:
            out.append(None)
        else:
            off = GRAD_OFFSET.get(i, 0)
            out.append((scale * torch.randn(off + p.numel(), device="cuda", generator=g))[off:])
    return out


def _optimizer(ps, lr, **kw):
    from occdepth_amd import train_graph
    opt = train_graph.make_capturable(torch.optim.AdamW(ps, lr=lr, betas=BETAS, eps=EPS, weight_decay=WD, fused=True, **kw))
    p = ps[8]                                               # moments as views at the parameter's own odd offset
    opt.state[p] = {"step": torch.zeros((), dtype=torch.float32, device="cuda"),
                    "exp_avg": torch.zeros(3 + p.numel(), device="cuda")[3:],
                    "exp_avg_sq": torch.zeros(3 + p.numel(), device="cuda")[3:]}
    return opt


class _Float64:
    """Accumulate, clip_grad_norm_ and AdamW in float64 (torch/nn/utils/clip_grad.py, torch/optim/adamw.py); max_norm None =
    no clipping."""

    def __init__(self, ps):
        self.p = [p.detach().double() for p in ps]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.acc = [None] * len(ps)
        self.t = [0] * len(ps)

    def micro(self, grads, first, n):
        for i, g in enumerate(grads):
            if g is not None:
                self.acc[i] = g.double() / n if first else self.acc[i] + g.double() / n

    def close(self, lr, max_norm):
        gs = self.acc
        total = torch.sqrt(sum((g * g).sum() for g in gs if g is not None))
        coef = 1.0 if max_norm is None else torch.clamp(max_norm / (total + 1e-6), max=1.0)
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


def _bits(ps, opt, w):
    """Everything a closing step writes: parameters, optimizer state, the window's norm scalars."""
    return ([p.detach().clone() for p in ps],
            [{k: v.clone() for k, v in opt.state[p].items()} for p in ps],
            None if w is None or w.norm is None else w.norm.clone())


def _assert_unchanged(before, after, what):
    (p0, s0, n0), (p1, s1, n1) = before, after
    assert all(torch.equal(a, b) for a, b in zip(p0, p1)), what
    for a, b in zip(s0, s1):
        if a:
            assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a), what
        else:                                               # state created by this call: "never stepped"
            assert all(float(v.abs().max()) == 0.0 for v in b.values()), what
    if n0 is not None:
        assert torch.equal(n0, n1), what
    elif n1 is not None:
        assert float(n1.abs().max()) == 0.0, what


def _run(which, max_norm, n=3, windows=2, flags=None, bad=None):
    """`windows` windows of `n` micro-batches, the device lr changed between the first two.  `which`: "float64", "torch",
    "kernels" (`flags`: GradWindow(device_flags=...)) or "plain" (n == 1 only: clip_adamw_step without a window).
    `bad`: (micro-batch, value) written into one gradient element.  Returns per-window norms, the parameters, the
    optimizer and the parameter list."""
    from occdepth_amd import optim
    ps = _tensors()
    opt = _optimizer(ps, 1e-3)
    ref = _Float64(ps) if which == "float64" else None
    w = optim.GradWindow(opt, n, device_flags=flags) if which == "kernels" else None
    acc = [None] * len(ps)
    norms = []
    for win in range(windows):
        if win == 1:
            opt.param_groups[0]["lr"].fill_(4e-4)
        for k in range(n):
            micro = win * n + k
            grads = _grad_values(ps, micro)
            if bad is not None and bad[0] == micro:
                grads[3][17] = bad[1]
            first, last = k == 0, k == n - 1
            if which == "float64":
                ref.micro(grads, first, n)
                if last:
                    norms.append(ref.close(float(opt.param_groups[0]["lr"]), max_norm))
            elif which == "torch":
                for i, g in enumerate(grads):
                    if g is None:
                        continue
                    if first:
                        acc[i] = g / n
                    else:
                        acc[i] += g / n
                if last:
                    for p, a in zip(ps, acc):
                        p.grad = a
                    if max_norm is not None:
                        norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
                    opt.step()
            else:
                for p, g in zip(ps, grads):
                    p.grad = g
                keep = [None if g is None else g.clone() for g in grads]
                before = _bits(ps, opt, w)
                if w is None:
                    norm = optim.clip_adamw_step(opt, max_norm)
                else:
                    w.set(first, last)
                    norm = optim.clip_adamw_step(opt, max_norm, window=w)
                same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))      # bits: a NaN equals itself
                assert all(k_ is None or (p.grad is g and same(k_, g)) for k_, p, g in zip(keep, ps, grads)), \
                    "p.grad must stay what the backward wrote"
                assert (norm is None) == (max_norm is None)
                if not last:
                    _assert_unchanged(before, _bits(ps, opt, w), (win, k))
                elif norm is not None:
                    norms.append(float(norm))
    return norms, (ref.p if ref else [p.detach().double() for p in ps]), opt, ps


def _same_bits(a, b):
    assert a[0] == b[0] or all(x != x and y != y for x, y in zip(a[0], b[0])), (a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))
    for p, q in zip(a[3], b[3]):
        assert a[2].state[p].keys() == b[2].state[q].keys()
        for k, v in a[2].state[p].items():
            assert torch.equal(v, b[2].state[q][k]), k


_SHARED = {}


def _shared(key, *args, **kw):
    """One computation per (run, clip) for all tests of this file; the results are not modified."""
    if key not in _SHARED:
        _SHARED[key] = _run(*args, **kw)
    return _SHARED[key]


def _max_norm(setting):
    n64 = _shared(("float64", None), "float64", None)[0][0]
    return {"inactive": 4.0 * n64, "active": 0.5 * n64}[setting]


@pytest.mark.parametrize("setting", ["inactive", "active"])
def test_accumulating_kernels_against_float64_with_torch_as_yardstick(setting, hip_lib):
    """N = 3, two windows, device lr changed between them, max_norm at four times and at half the first window's norm.  The
    kernels' error against the float64 emulation is at most 2x that of torch's float32 sequence on the same inputs, for
    total_norm (largest error over the windows) and for the final parameters (largest absolute error over all tensors) --
    the bound of test_clip_adamw_gpu.py::test_kernels_against_float64_with_torch_as_yardstick; torch's error is not zero.
    `step` is 2.0 (windows, not micro-batches); `_run` checks that p.grad keeps its bits over every call and that p, m, v,
    step and the norm scalars keep theirs over every non-closing call."""
    max_norm = _max_norm(setting)
    norm64, p64, _, _ = _shared(("float64", setting), "float64", max_norm)
    norm_t, p_t, opt_t, ps_t = _shared(("torch", setting), "torch", max_norm)
    norm_k, p_k, opt_k, ps_k = _shared(("kernels", setting), "kernels", max_norm)
    assert len(norm64) == len(norm_t) == len(norm_k) == 2
    err = lambda a, b: max(float((x - y).abs().max()) for x, y in zip(a, b))
    e_norm_t = max(abs(a - b) for a, b in zip(norm_t, norm64))
    e_norm_k = max(abs(a - b) for a, b in zip(norm_k, norm64))
    e_p_t, e_p_k = err(p_t, p64), err(p_k, p64)
    print(f"{setting}: total_norm {norm64!r} max_norm {max_norm:.6g}; |total_norm - f64| torch {e_norm_t:.3e} kernels "
          f"{e_norm_k:.3e}; max |p - f64| torch {e_p_t:.3e} kernels {e_p_k:.3e}")
    assert e_norm_t > 0.0 and e_p_t > 0.0                   # the bound below is not vacuous
    assert e_norm_k <= 2.0 * e_norm_t, (e_norm_k, e_norm_t)
    assert e_p_k <= 2.0 * e_p_t, (e_p_k, e_p_t)
    for i, (a, b) in enumerate(zip(ps_k, ps_t)):
        if i == NO_GRAD:
            assert len(opt_k.state[a]) == 0 and len(opt_t.state[b]) == 0 and torch.equal(a, b)
            continue
        assert float(opt_k.state[a]["step"]) == 2.0 and float(opt_t.state[b]["step"]) == 2.0, i
        for k in ("exp_avg", "exp_avg_sq"):
            x, y = opt_k.state[a][k], opt_t.state[b][k]
            assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max()) + 1e-30, (i, k)
    assert set(opt_k.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}     # accumulators stay out of checkpoints


def test_device_flags_host_flags_and_two_runs_are_bit_identical(hip_lib):
    max_norm = _max_norm("active")
    host = _shared(("kernels", "active"), "kernels", max_norm)
    _same_bits(host, _run("kernels", max_norm, flags=True))
    _same_bits(host, _run("kernels", max_norm, flags=False))
    _same_bits(host, _run("kernels", max_norm))
    # without clipping too (no norm comes back)
    free = _run("kernels", None)
    _same_bits(free, _run("kernels", None, flags=True))
    assert free[0] == []


@pytest.mark.parametrize("max_norm", [3.0, 1e30])
def test_window_of_one_is_the_plain_step_bit_for_bit(max_norm, hip_lib):
    """N = 1 (first = last = True): parameters, moments, `step` and the norm of four steps equal `clip_adamw_step` without a
    window."""
    a = _run("kernels", max_norm, n=1, windows=4)
    b = _run("plain", max_norm, n=1, windows=4)
    assert len(a[0]) == 4
    _same_bits(a, b)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_in_a_window_gives_torchs_pattern(bad, hip_lib):
    """The second micro-batch of the second window of two brings one Inf element: the accumulator holds Inf, total_norm
    Inf, clip_coef 0, that element's product NaN -> exactly one parameter element NaN.  One NaN element: total_norm and
    clip_coef NaN -> every stepped parameter NaN.  Without clipping (coefficient exactly 1, no norm) an Inf gradient gives
    the pattern of torch's unclipped step: the one element."""
    n_stepped = sum(SIZES) + 5001 + 9001 + CHUNK + 3 + CHUNK + 5
    for max_norm in (1.0, None):
        if max_norm is None and bad != bad:
            continue
        t = _run("torch", max_norm, n=2, bad=(3, bad))
        k = _run("kernels", max_norm, n=2, bad=(3, bad))
        for x, y in zip(t[0], k[0]):
            assert x == y or (x != x and y != y) or abs(x - y) <= 1e-5 * abs(x), (t[0], k[0])
        assert all(torch.equal(torch.isfinite(x), torch.isfinite(y)) and torch.equal(torch.isnan(x), torch.isnan(y))
                   for x, y in zip(t[1], k[1]))
        n_bad = sum(int((~torch.isfinite(x)).sum()) for x in k[1])
        assert n_bad == (1 if bad == float("inf") else n_stepped), (max_norm, n_bad)


def test_captured_accumulating_step_replays_like_the_eager_kernels(hip_lib):
    """A hipGraph around `clip_adamw_step(opt, c, window=w)` alone, static gradient tensors: six replays (two windows of
    three), the new gradient values copied in and the position set before each, give the bits of the eager kernel run of
    the error test -- through the device flags, one capture serves every position.  Nothing to zero: the capture holds no
    memset node that had to be rewritten."""
    from occdepth_amd import optim, train_graph
    max_norm = _max_norm("active")
    eager = _shared(("kernels", "active"), "kernels", max_norm)
    ps = _tensors()
    opt = _optimizer(ps, 1e-3)
    w = optim.GradWindow(opt, 3)
    static = _grad_values(ps, 0)
    for p, g in zip(ps, static):
        p.grad = g
        if g is not None and len(opt.state[p]) == 0:       # as torch creates it for a capturable AdamW
            opt.state[p] = {"step": torch.zeros((), dtype=torch.float32, device="cuda"),
                            "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    optim.prepare_capture(opt, w)
    torch.cuda.synchronize()
    graph = train_graph.new_graph()
    with torch.cuda.graph(graph, capture_error_mode=train_graph.CAPTURE_MODE):
        norm = optim.clip_adamw_step(opt, max_norm, window=w)
    assert train_graph.seal_graph(graph) == 0
    keep = optim.live_tables(opt, w)
    assert any(t is w.flags for t in keep) and all(any(t is a for t in keep) for a in w.acc.values())
    start = _bits(ps, opt, w)
    torch.cuda.synchronize()
    _assert_unchanged(start, _bits(ps, opt, w), "capture")
    norms = []
    for micro in range(6):
        if micro == 3:
            opt.param_groups[0]["lr"].fill_(4e-4)
        for s, g in zip(static, _grad_values(ps, micro)):
            if s is not None:
                s.copy_(g)
        before = _bits(ps, opt, w)
        w.set(micro % 3 == 0, micro % 3 == 2)
        graph.replay()
        if micro % 3 == 2:
            norms.append(float(norm))
        else:
            _assert_unchanged(before, _bits(ps, opt, w), micro)
    _same_bits(eager, (norms, [p.detach().double() for p in ps], opt, ps))


# ------------------------------------------------------------------------------------------------ the training step
def _clone_batch(batch):
    return {k: ([t.clone() if torch.is_tensor(t) else t for t in v] if isinstance(v, (list, tuple))
                else (v.clone() if torch.is_tensor(v) else v)) for k, v in batch.items()}


def _decoder_param(m):
    return next(iter(m.net_3d_decoder.parameters())).detach().float().cpu().clone()


def test_whole_accumulating_step_hipgraph_matches_eager_gpu(hip_lib):
    """GraphedTrainStep(grad_clip=c, accumulate=2), c = half the norm of the first eager step, on the reduced SemanticKITTI
    model in training mode, optimizer settings of test_clip_adamw_gpu.py (the update depends on the gradient's scale).
    Capturing trains nothing.  Four replays = two windows: after replays 0 and 2 every parameter keeps its bits, after 1 and
    3 they moved, `step` ends at 2.0.  Against the eager torch sequence (two backwards of loss / 2 into p.grad,
    clip_grad_norm_, opt.step()) the bounds are those of test_train_step.py::test_whole_step_hipgraph_matches_eager_gpu: 1e-5
    on the first loss, 1.5e-2 on later losses, 5e-3 on the first decoder parameter."""
    from occdepth_amd import train_graph
    from test_clip_adamw_gpu import EPS_OVER_RMS, LR, _first_norm
    from test_lightning_hooks import _gpu_frames
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, frames = _gpu_frames("kitti_small", 4)
    norm, n_elems = _first_norm(m0, frames[0])
    c, eps = 0.5 * norm, EPS_OVER_RMS * norm / n_elems ** 0.5
    assert c > 0

    def setup():
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        return m, train_graph.make_capturable(torch.optim.AdamW(m.parameters(), lr=LR, eps=eps, fused=True))

    # eager torch sequence
    m, opt = setup()
    le, ne = [], []
    for i, frame in enumerate(frames):
        if i % 2 == 0:
            opt.zero_grad(set_to_none=True)
        loss = m.training_step(frame, 0)
        (loss / 2).backward()
        le.append(float(loss.detach()))
        if i % 2 == 1:
            ne.append(float(torch.nn.utils.clip_grad_norm_(m.parameters(), c)))
            opt.step()
    pe = _decoder_param(m)
    assert m.cur_batch == 4

    # captured
    m, opt = setup()
    gs = train_graph.GraphedTrainStep(m, opt, _clone_batch(frames[0]), warmup=2, grad_clip=c, accumulate=2)
    assert gs.window is not None and gs.window.n == 2
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    assert gs.capture(), gs.error
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "capture must not train"
    assert m.cur_batch == 0 and m.train_metrics.count == 1e-8
    assert all(float(v.abs().max()) == 0.0 for st in opt.state.values() for v in st.values() if torch.is_tensor(v))
    assert m.train_metrics.hist is None or int(m.train_metrics.hist.sum()) == 0
    assert all(float(a.abs().max()) == 0.0 for a in gs.window.acc.values()) and not gs.window.is_open
    lg, ng = [], []
    for i, frame in enumerate(frames):
        gs.load_batch(frame)
        gs.window.set(i % 2 == 0, i % 2 == 1)
        params = [p.detach().clone() for p in m.parameters()]
        lg.append(float(gs()))
        same = [torch.equal(a, b) for a, b in zip(params, m.parameters())]
        if i % 2 == 0:
            assert all(same), i
        else:
            assert not any(same[:1]) and sum(same) < len(same) // 2, (i, sum(same), len(same))
            ng.append(float(m.logged["train/grad_norm"]))
    pg = _decoder_param(m)
    assert m.cur_batch == 4
    assert all(float(st["step"]) == 2.0 for st in opt.state.values() if len(st))
    print("clip", c, "eps", eps, "eager", le, ne, "graph", lg, ng)
    print("eager vs graph: losses", [abs(a - b) / abs(a) for a, b in zip(le, lg)], "parameter",
          float((pe - pg).abs().max() / pe.abs().max()))
    assert all(n > c for n in ng) and all(n > c for n in ne)
    assert abs(le[0] - lg[0]) <= 1e-5 * abs(le[0]), (le, lg)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(le, lg)), (le, lg)
    assert float((pe - pg).abs().max() / pe.abs().max()) < 5e-3


class AccumTrainer:
    """pytorch-lightning 1.4.9's loop for fit with `Trainer(gradient_clip_val=..., accumulate_grad_batches=N)`.  Automatic
    optimisation: training_step, backward of loss / N, and when the window closes -- (batch_idx + 1) % N == 0 or the epoch's
    last batch (TrainingBatchLoop.should_accumulate) -- clip_grad_norm_, optimizer.step, zero_grad.  Manual optimisation:
    training_step alone; the module reads the trainer's settings."""

    def __init__(self, model, gradient_clip_val, accumulate_grad_batches, num_training_batches):
        self.model, self.gradient_clip_val, self.gradient_clip_algorithm = model, gradient_clip_val, "norm"
        self.accumulate_grad_batches, self.num_training_batches = accumulate_grad_batches, num_training_batches
        self.logged = {}
        model.log = lambda key, value, **kw: self.logged.__setitem__(key, float(value))
        model.trainer = self

    def fit(self, batches):
        assert len(batches) == self.num_training_batches
        (opt,), _ = self.model.configure_optimizers()
        n = self.accumulate_grad_batches
        self.losses, self.norms = [], []
        self.model.on_train_epoch_start()
        opt.zero_grad()
        for i, b in enumerate(batches):
            closes = (i + 1) % n == 0 or i + 1 == self.num_training_batches
            if getattr(self.model, "automatic_optimization", True):
                loss = self.model.training_step(b, i)
                (loss / n).backward()
                if closes:
                    self.norms.append(float(torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.gradient_clip_val)))
                    opt.step()
                    opt.zero_grad()
            else:
                loss = self.model.training_step(b, i)
                assert not loss.requires_grad
                if closes:
                    self.norms.append(self.logged["train/grad_norm"])
            self.losses.append(float(loss.detach()))
            self.model.on_train_batch_end(None, b, i, 0)


def test_fast_train_accumulates_like_the_trainer_gpu(hip_lib, monkeypatch):
    """An unmodified scripts/train.py with OCCDEPTH_FAST_TRAIN=1 and a Trainer that accumulates over two batches: the fast
    path (captured step, three frames: a full window and the epoch's short last one) trains like the same module under
    automatic optimisation, within the bounds of test_whole_step_hipgraph_matches_eager_gpu."""
    from test_clip_adamw_gpu import _first_norm
    from test_lightning_hooks import _gpu_frames
    monkeypatch.delenv("OCCDEPTH_FAST_TRAIN_ACCUM", raising=False)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, frames = _gpu_frames("kitti_small", 3)
    c = 0.25 * _first_norm(m0, frames[0])[0]                # the short last window's gradient is half a frame's
    runs = {}
    for name in ("plain", "fast"):
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        if name == "fast":
            m.enable_fast_train()
        tr = AccumTrainer(m, c, 2, 3)
        tr.fit(frames)
        runs[name] = (tr.losses, _decoder_param(m), tr.norms)
        assert m.cur_batch == 3
        if name == "fast":
            st = m._fast_train
            assert st["graph"] is not None and st["graph"].graph is not None, getattr(st["graph"], "error", None)
            assert st["graph"].grad_clip == c and st["graph"].window is st["window"] and st["window"].n == 2
            assert all(float(s["step"]) == 2.0 for s in m._opt.state.values() if len(s))
    (lp, pp, np_), (lf, pf, nf) = runs["plain"], runs["fast"]
    print("plain", lp, np_, "fast", lf, nf)
    assert len(np_) == len(nf) == 2 and all(n > c for n in np_) and all(n > c for n in nf)
    assert abs(lp[0] - lf[0]) <= 1e-5 * abs(lp[0]), (lp, lf)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(lp, lf)), (lp, lf)
    assert float((pp - pf).abs().max() / pp.abs().max()) < 5e-3
