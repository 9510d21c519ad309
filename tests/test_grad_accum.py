"""CPU: gradient accumulation in the fast training step (optim.GradWindow behind `clip_adamw_step(window=...)`, the wiring
in train_graph.py and models/OccDepth.py).  On CPU tensors the window runs torch's own sequence on its accumulators --
`p.grad = g0 / n; p.grad += g1 / n; ...; clip_grad_norm_; AdamW.step()` -- so every comparison here is exact.  The HIP
kernels are covered by tests/test_grad_accum_gpu.py."""
import copy
import types

import pytest
import torch

import emu
from test_clip_adamw import _cpu_train_setup, _params, _same, _set_grads
from test_oracle_vs_golden import build_product

N = 3
SKIP = 2


def _state_bits(params, opt):
    return [(p.detach().clone(), {k: torch.as_tensor(v).clone() for k, v in opt.state[p].items()}) for p in params]


def _equal_bits(a, b):
    return all(torch.equal(pa, pb) and sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)
               for (pa, sa), (pb, sb) in zip(a, b))


@pytest.mark.parametrize("max_norm", [1.0, 1e3, None], ids=["norm_above_max", "norm_below_max", "no_clip"])
def test_window_step_equals_torchs_accumulation_sequence_cpu(max_norm):
    """Two windows of three micro-batches, one parameter without a gradient.  After a non-closing call parameters and
    optimizer state keep their bits; after a closing call parameters, moments, `step` and the returned norm equal the torch
    sequence on a deep copy; `step` counts windows; without a clip value the window still accumulates (no norm returned)."""
    from occdepth_amd import optim
    mine, ref = _params(), _params()
    opt_m = torch.optim.AdamW(mine, lr=1e-2, weight_decay=0.05)
    opt_r = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.05)
    w = optim.GradWindow(opt_m, N)
    plain = _params()                                       # a step per micro-batch: what the parent commit does
    opt_p = torch.optim.AdamW(plain, lr=1e-2, weight_decay=0.05)
    for window in range(2):
        for k in range(N):
            step = window * N + k
            _set_grads(mine, step, 10.0, SKIP)
            _set_grads(ref, step, 10.0, SKIP)
            _set_grads(plain, step, 10.0, SKIP)
            optim.clip_adamw_step(opt_p, max_norm)
            micro = [None if p.grad is None else p.grad.clone() for p in ref]
            before = _state_bits(mine, opt_m)
            w.set(k == 0, k == N - 1)
            assert w.is_open == (k != N - 1)
            got = optim.clip_adamw_step(opt_m, max_norm, window=w)
            # the torch sequence
            for p, g in zip(ref, micro):
                if g is None:
                    continue
                if k == 0:
                    p.grad = g / N
                else:
                    p.grad = acc[id(p)]
                    p.grad += g / N
            acc = {id(p): p.grad for p in ref if p.grad is not None}
            if k < N - 1:
                assert _equal_bits(before, _state_bits(mine, opt_m)), (window, k)
                if window == 0:
                    assert got is None                      # no window closed yet
                continue
            if max_norm is not None:
                want = torch.nn.utils.clip_grad_norm_(ref, max_norm)
                assert torch.equal(got, want), (window, float(got), float(want))
                assert (float(want) > max_norm) == (max_norm == 1.0)
            else:
                assert got is None
            opt_r.step()
            assert not _equal_bits(before, _state_bits(mine, opt_m))
            for i, (a, b) in enumerate(zip(mine, ref)):
                assert torch.equal(a, b), (window, i)
                if i == SKIP:
                    assert len(opt_m.state[a]) == 0 and torch.equal(a, _params()[i])
                    continue
                for key in ("step", "exp_avg", "exp_avg_sq"):
                    assert torch.equal(torch.as_tensor(opt_m.state[a][key]), torch.as_tensor(opt_r.state[b][key])), (i, key)
                assert float(opt_m.state[a]["step"]) == window + 1          # windows, not micro-batches
    assert not all(torch.equal(a, b) for a, b in zip(mine, plain))
    assert set(opt_m.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}     # accumulators live outside opt.state


def test_window_arguments_cpu():
    from occdepth_amd import optim, train_graph
    import inspect
    ps = _params()
    opt = torch.optim.AdamW(ps, lr=1e-2)
    for bad in (0, -1, 2.5, True, {4: 2}, None):
        with pytest.raises(ValueError):
            optim.GradWindow(opt, bad)
    w = optim.GradWindow(torch.optim.AdamW(_params(), lr=1e-2), 2)
    _set_grads(ps, 0, 1.0, None)
    with pytest.raises(ValueError, match="another optimizer"):
        optim.clip_adamw_step(opt, 1.0, window=w)
    # a window of one is the plain step
    a, b = _params(), _params()
    oa, ob = torch.optim.AdamW(a, lr=1e-2), torch.optim.AdamW(b, lr=1e-2)
    _set_grads(a, 0, 10.0, SKIP)
    _set_grads(b, 0, 10.0, SKIP)
    na = optim.clip_adamw_step(oa, 1.0, window=optim.GradWindow(oa, 1))
    nb = optim.clip_adamw_step(ob, 1.0)
    assert torch.equal(na, nb) and all(torch.equal(x, y) for x, y in zip(a, b))
    sig = inspect.signature(train_graph.GraphedTrainStep.__init__).parameters
    assert sig["accumulate"].default == 1
    gs = train_graph.GraphedTrainStep(torch.nn.Linear(2, 2), oa, {}, accumulate=1)
    assert gs.window is None
    gs = train_graph.GraphedTrainStep(torch.nn.Linear(2, 2), oa, {}, accumulate=4)
    assert gs.window.n == 4 and gs.window.opt is oa
    for bad in (0, 2.5, {0: 2}):
        with pytest.raises(ValueError):
            train_graph.GraphedTrainStep(torch.nn.Linear(2, 2), oa, {}, accumulate=bad)


# ---------------------------------------------------------------------------------------------- the model's fast step
def _three_batches(batch):
    g = torch.Generator().manual_seed(5)
    out = [batch]
    for _ in range(2):
        out.append(dict(batch, img=batch["img"] + 0.05 * torch.randn(batch["img"].shape, generator=g)))
    return out


def _hand_window(m, opt, batches, idxs, n, clip):
    """Backward of each loss, the gradients divided by n and added in order, [clip_grad_norm_], AdamW.step()."""
    params = list(m.parameters())
    acc = {}
    for k, (b, i) in enumerate(zip(batches, idxs)):
        opt.zero_grad(set_to_none=True)
        with emu.patched():
            m.training_step(b, i).backward()
        for p in params:
            if p.grad is None:
                continue
            if k == 0:
                acc[p] = p.grad / n
            else:
                acc[p] += p.grad / n
    for p in params:
        p.grad = acc.get(p)
    norm = None
    if clip:
        norm = torch.nn.utils.clip_grad_norm_(params, clip)
    opt.step()
    return norm


def test_manual_eager_step_accumulates_like_the_trainer_cpu():
    """`enable_fast_train` on the CPU with a trainer that asks for `accumulate_grad_batches=2` over an epoch of three batches:
    nothing moves after batch 0, the window [0, 1] closes after batch 1 and the epoch's last batch closes a window of one that
    is still scaled by 1/2 -- each equal, bit for bit, to the hand-written torch sequence.  One thread, as in
    test_clip_adamw.py::test_manual_eager_step_clips_like_the_trainer_cpu."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _check_accumulating_step()
    finally:
        torch.set_num_threads(threads)


def _check_accumulating_step():
    m0, batch = _cpu_train_setup("nyu_small")
    # the untrained model in eval mode (BatchNorm on its initial running statistics) survives one update of the default
    # 1e-4 per element but gives a NaN loss after it, and this test takes two: 1e-6 keeps every loss finite
    m0.lr = 1e-6
    batches = _three_batches(batch)
    probe = copy.deepcopy(m0)
    (opt,), _ = probe.configure_optimizers()
    clip = 0.5 * float(_hand_window(probe, opt, batches[:2], [0, 1], 2, 1e30))
    assert clip > 0
    for c in (clip, None):
        ref = copy.deepcopy(m0)
        (opt_r,), _ = ref.configure_optimizers()
        fast = copy.deepcopy(m0).enable_fast_train()
        fast.trainer = types.SimpleNamespace(gradient_clip_val=c, gradient_clip_algorithm="norm", accumulate_grad_batches=2,
                                             num_training_batches=3)
        fast.configure_optimizers()
        with emu.patched(), pytest.warns(UserWarning, match="needs the model on the GPU"):
            fast.training_step(batches[0], 0)
        assert _same(fast, m0) and "train/grad_norm" not in fast.logged
        assert fast._fast_train["window"].n == 2 and fast._fast_train["window"].is_open
        with emu.patched():
            fast.training_step(batches[1], 1)
        norm = _hand_window(ref, opt_r, batches[:2], [0, 1], 2, c)
        assert _same(fast, ref) and not _same(fast, m0)
        if c:
            assert float(norm) > c and torch.equal(fast.logged["train/grad_norm"], norm)
        else:
            assert "train/grad_norm" not in fast.logged
        assert not fast._fast_train["window"].is_open
        mid = copy.deepcopy(fast)
        with emu.patched():
            fast.training_step(batches[2], 2)
        norm = _hand_window(ref, opt_r, batches[2:], [2], 2, c)
        assert _same(fast, ref) and not _same(fast, mid)
        if c:
            assert torch.equal(fast.logged["train/grad_norm"], norm)
        assert fast.cur_batch == 3 and ref.cur_batch == 3
        assert all(bool(torch.isfinite(p).all()) for p in fast.parameters())
        assert all(float(s["step"]) == 2.0 for s in fast._opt.state.values())


def test_accumulate_resolution_order_cpu(monkeypatch):
    monkeypatch.delenv("OCCDEPTH_FAST_TRAIN_ACCUM", raising=False)
    m, _, _ = build_product("nyu_small")
    assert m._accumulate_value() == 1
    m.trainer = types.SimpleNamespace(gradient_clip_val=35)             # a trainer without the attribute
    assert m._accumulate_value() == 1
    m.trainer = types.SimpleNamespace(accumulate_grad_batches=4)
    assert m._accumulate_value() == 4
    monkeypatch.setenv("OCCDEPTH_FAST_TRAIN_ACCUM", "3")
    assert m._accumulate_value() == 3
    m.enable_fast_train(accumulate=2)
    assert m._accumulate_value() == 2
    m.enable_fast_train()
    assert m._accumulate_value() == 3
    for bad in ("0", "2.5", "four"):
        monkeypatch.setenv("OCCDEPTH_FAST_TRAIN_ACCUM", bad)
        with pytest.raises(ValueError, match="OCCDEPTH_FAST_TRAIN_ACCUM"):
            m._accumulate_value()
    monkeypatch.delenv("OCCDEPTH_FAST_TRAIN_ACCUM")
    for bad in (0, 2.5, {0: 2, 4: 1}):
        with pytest.raises(ValueError):
            m.enable_fast_train(accumulate=bad)
        m.trainer = types.SimpleNamespace(accumulate_grad_batches=bad)
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            m._accumulate_value()
    m.trainer = None
    assert m._accumulate_value() == 1


def test_accumulate_is_fixed_at_the_first_fast_step_cpu(monkeypatch):
    monkeypatch.delenv("OCCDEPTH_FAST_TRAIN_ACCUM", raising=False)
    m0, batch = _cpu_train_setup("nyu_small")
    m = copy.deepcopy(m0).enable_fast_train(accumulate=2)
    m.configure_optimizers()
    with emu.patched(), pytest.warns(UserWarning, match="needs the model on the GPU"):
        m.training_step(batch, 0)
    m.fast_train_accumulate = 3
    with emu.patched(), pytest.raises(ValueError, match="changed from 2 to 3"):
        m.training_step(batch, 1)
