"""CPU: gradient-norm clipping in the fast training step (occdepth_amd/optim.py, the wiring in train_graph.py and
models/OccDepth.py).  On CPU tensors `clip_adamw_step` IS torch's sequence -- `clip_grad_norm_` + `AdamW.step()` -- so
every comparison here is exact.  The HIP kernels are covered by tests/test_clip_adamw_gpu.py."""
import copy
import os
import socket
import types

import pytest
import torch

import emu
import golden_cases as gc
from test_oracle_vs_golden import build_product


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = [(1,), (7,), (33, 5), (4097,), (3, 4, 5, 6)]
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]


def _set_grads(params, step, scale, skip):
    g = torch.Generator().manual_seed(100 + step)
    for i, p in enumerate(params):
        p.grad = None if i == skip else scale * torch.randn(p.shape, generator=g)


@pytest.mark.parametrize("scale", [0.01, 10.0], ids=["norm_below_max", "norm_above_max"])
def test_clip_adamw_step_equals_clip_grad_norm_then_adamw_cpu(scale):
    """Three steps with weight decay and one parameter that never gets a gradient: parameters, moments, step counters and
    the returned norm equal `clip_grad_norm_(params, max_norm)` + `AdamW.step()` on a deep copy, bit for bit; the
    gradient-less parameter has no state and does not move."""
    from occdepth_amd import optim
    max_norm, skip = 1.0, 2
    mine, ref = _params(), _params()
    opt_m = torch.optim.AdamW(mine, lr=1e-2, weight_decay=0.05)
    opt_r = torch.optim.AdamW(ref, lr=1e-2, weight_decay=0.05)
    for step in range(3):
        _set_grads(mine, step, scale, skip)
        _set_grads(ref, step, scale, skip)
        n_m = optim.clip_adamw_step(opt_m, max_norm)
        n_r = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt_r.step()
        assert torch.equal(n_m, n_r)
        assert (float(n_r) > max_norm) == (scale > 1.0)
    for i, (a, b) in enumerate(zip(mine, ref)):
        assert torch.equal(a, b), i
        if i == skip:
            assert len(opt_m.state[a]) == 0 and torch.equal(a, _params()[i])
            continue
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(opt_m.state[a][k]), torch.as_tensor(opt_r.state[b][k])), (i, k)
    # a later plain step on the same optimizer keeps working (torch's state keys)
    _set_grads(mine, 3, scale, skip)
    opt_m.step()


def test_no_clip_value_is_a_plain_step_and_sparse_gradients_raise_cpu():
    from occdepth_amd import optim
    for none in (None, 0, 0.0):
        mine, ref = _params(), _params()
        opt_m, opt_r = torch.optim.AdamW(mine, lr=1e-2), torch.optim.AdamW(ref, lr=1e-2)
        _set_grads(mine, 0, 10.0, 1)
        _set_grads(ref, 0, 10.0, 1)
        assert optim.clip_adamw_step(opt_m, none) is None
        opt_r.step()
        assert all(torch.equal(a, b) for a, b in zip(mine, ref))
        assert all(torch.equal(a.grad, b.grad) for a, b in zip(mine, ref) if a.grad is not None)
    emb = torch.nn.Embedding(8, 4, sparse=True)
    opt = torch.optim.AdamW(emb.parameters(), lr=1e-2)
    emb(torch.tensor([1, 3])).sum().backward()
    with pytest.raises(RuntimeError, match="sparse"):
        optim.clip_adamw_step(opt, 1.0)
    out = torch.zeros(())
    mine = _params()
    opt = torch.optim.AdamW(mine, lr=1e-2)
    _set_grads(mine, 0, 1.0, None)
    want = torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in mine]))
    assert optim.clip_adamw_step(opt, 1.0, out_norm=out) is out and torch.equal(out, want)


# ---------------------------------------------------------------------------------------------- the model's fast step
def _cpu_train_setup(cfg_name):
    """The reduced model in eval mode (BatchNorm on running statistics) with a complete training batch, on the CPU."""
    m, cfg, _ = build_product(cfg_name)
    m.eval()
    batch = gc.occdepth_batch(cfg_name)
    with torch.no_grad(), emu.patched():
        out = m(batch)
    shapes = {k: tuple(v.shape) for k, v in out.items() if torch.is_tensor(v)}
    batch = dict(batch, **gc.train_extras(cfg_name, shapes, tuple(cfg.full_scene_size), cfg.n_classes, batch["img"].shape[-2:]))
    return m, batch


def _hand_step(m, batch, clip):
    """zero_grad, training_step, backward, [clip_grad_norm_], AdamW.step(): what Lightning's automatic optimisation does."""
    (opt,), _ = m.configure_optimizers()
    opt.zero_grad()
    with emu.patched():
        loss = m.training_step(batch, 0)
        loss.backward()
    params = list(m.parameters())
    norm = torch.linalg.vector_norm(torch.stack([p.grad.norm() for p in params if p.grad is not None]))
    if clip:
        assert torch.equal(torch.nn.utils.clip_grad_norm_(params, clip), norm)
    opt.step()
    return float(norm)


def _fast_step(m, batch):
    m.configure_optimizers()
    with emu.patched(), pytest.warns(UserWarning, match="needs the model on the GPU"):
        m.training_step(batch, 0)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.parameters(), b.parameters()))


def test_manual_eager_step_clips_like_the_trainer_cpu():
    """`enable_fast_train` on the CPU runs `_manual_eager_step`.  With a clip of half the measured first-step norm its
    parameters equal the hand-written torch sequence (clip_grad_norm_ between backward and AdamW.step) and differ from the
    unclipped step; the value comes from `enable_fast_train(grad_clip=...)` first, else from the attached trainer's
    `gradient_clip_val`; 0 / None / no trainer leave the step the unclipped one; clipping by value raises.
    One thread: the comparisons are exact, and ATen's multi-threaded CPU backward does not always add in the same order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _check_manual_eager_step()
    finally:
        torch.set_num_threads(threads)


def _check_manual_eager_step():
    m0, batch = _cpu_train_setup("nyu_small")
    plain = copy.deepcopy(m0)
    norm = _hand_step(plain, batch, None)
    clip = 0.5 * norm
    assert clip > 0
    clipped = copy.deepcopy(m0)
    assert _hand_step(clipped, batch, clip) == norm
    assert not _same(plain, clipped)

    def fast(grad_clip=None, trainer=None):
        m = copy.deepcopy(m0).enable_fast_train(grad_clip=grad_clip)
        if trainer is not None:
            m.trainer = trainer
        _fast_step(m, batch)
        return m

    a = fast(grad_clip=clip)
    assert _same(a, clipped) and not _same(a, plain)
    assert float(a.logged["train/grad_norm"]) == norm
    b = fast(trainer=types.SimpleNamespace(gradient_clip_val=clip, gradient_clip_algorithm="norm"))
    assert _same(b, clipped) and float(b.logged["train/grad_norm"]) == norm
    # first hit wins: the explicit argument, 0 included, beats the trainer's value
    c = fast(grad_clip=0, trainer=types.SimpleNamespace(gradient_clip_val=clip))
    assert _same(c, plain) and "train/grad_norm" not in c.logged
    for tr in (None, types.SimpleNamespace(gradient_clip_val=0), types.SimpleNamespace(gradient_clip_val=None),
               types.SimpleNamespace()):
        d = fast(trainer=tr)
        assert _same(d, plain) and "train/grad_norm" not in d.logged


def test_clip_value_resolution_order_cpu():
    m, _, _ = build_product("nyu_small")
    assert m._grad_clip_value() is None
    m.trainer = types.SimpleNamespace(gradient_clip_val=35, gradient_clip_algorithm="norm")
    assert m._grad_clip_value() == 35.0
    m.enable_fast_train(grad_clip=7.0)
    assert m._grad_clip_value() == 7.0
    m.enable_fast_train(grad_clip=0)
    assert m._grad_clip_value() is None
    m.enable_fast_train()
    assert m._grad_clip_value() == 35.0
    m.trainer = types.SimpleNamespace(gradient_clip_val=35, gradient_clip_algorithm="value")
    with pytest.raises(NotImplementedError, match="global norm"):
        m._grad_clip_value()
    m.trainer = types.SimpleNamespace(gradient_clip_val=0.0, gradient_clip_algorithm="value")     # nothing to clip
    assert m._grad_clip_value() is None
    from occdepth_amd import train_graph
    import inspect
    assert inspect.signature(train_graph.GraphedTrainStep.__init__).parameters["grad_clip"].default is None


# ---------------------------------------------------------------------------------------------- several ranks (gloo)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, q):
    import torch.distributed as dist
    from occdepth_amd import optim, shard
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4))
    opt = torch.optim.AdamW(net.parameters(), lr=1e-2, weight_decay=0.01)
    buckets = shard.GradBuckets(net.parameters(), dist)
    norms = []
    for step in range(2):
        buckets.zero_grad()
        x = torch.randn(8, 16, generator=torch.Generator().manual_seed(10 * step + rank))      # every rank its own data
        (net(x) ** 2).sum().backward()
        buckets.finish()
        norms.append(optim.clip_adamw_step(opt, 0.5).clone())
    q.put((rank, [n.numpy().tobytes() for n in norms], [p.detach().numpy().tobytes() for p in net.parameters()]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_clip_the_same_norm_after_the_gradient_average_gloo():
    """Several ranks: the clip follows `buckets.finish()`, so every rank measures the norm of the AVERAGED gradients -- the
    same bits on both ranks -- and the replicas stay identical.  This is the torch sequence on CPU tensors over gloo (the
    two-process GPU harness of tests/syncbn_ddp_worker.py drives a whole model and is not reusable from a new worker
    without editing it); the kernels' own run-to-run determinism is checked in tests/test_clip_adamw_gpu.py."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (n, w)) for r, n, w in (q.get(timeout=120) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0][0] == got[1][0] and got[0][1] == got[1][1]
    first = torch.frombuffer(bytearray(got[0][0][0]), dtype=torch.float32)
    assert float(first) > 0.5                              # the clip was active
