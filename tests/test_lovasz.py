"""Lovasz-softmax loss and the K38 sort, without a GPU: the exports, the float64 restatement against brute force, the closed
form of the Jaccard increment against the cumsum differences, the torch formulation against the restatement, edge cases,
host logic.  The cases and restatements below are shared with test_lovasz_gpu.py."""
import ctypes
import functools
import sys

import numpy as np
import pytest
import torch

Q = 60
ONE_BITS = 0x3F800000


# ------------------------------------------------------------------------------------------------------- restatements
def closed_form(err, fg, valid):
    """The specification's closed form in numpy: err (C, N) float32, fg (C, N) bool, valid (N,) bool ->
    (q (C, N) float32: (fg ? -g : g) at valid voxels, 0 elsewhere; loss_q (C,) int64: sum of rint(e g 2^60); G (C,)).
    Stable descending order, integer counters, one IEEE float64 division, g rounded once to float32."""
    err, fg, valid = np.asarray(err, np.float32), np.asarray(fg, bool) & np.asarray(valid, bool)[None], np.asarray(valid, bool)
    C, N = err.shape
    q, loss_q, G = np.zeros((C, N), np.float32), np.zeros(C, np.int64), np.zeros(C, np.int64)
    idx = np.flatnonzero(valid)
    for c in range(C):
        e, f = err[c, idx], fg[c, idx]
        order = np.argsort(-e, kind="stable")
        e, f = e[order].astype(np.float64), f[order]
        G[c] = g_total = int(f.sum())
        if g_total == 0:
            continue
        fg_incl = np.cumsum(f).astype(np.int64)
        F = fg_incl - f                                        # foreground strictly before
        b = np.arange(1, len(f) + 1, dtype=np.int64) - fg_incl  # background up to and including
        tot = (g_total + b).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(f, 1.0 / tot, (g_total - F).astype(np.float64) / ((g_total + b - 1).astype(np.float64) * tot))
        loss_q[c] = int(np.rint(e * g * float(1 << Q)).astype(np.int64).sum())
        q[c, idx[order]] = np.where(f, -g, g).astype(np.float32)
    return q, loss_q, G


def brute_force(err, fg, valid):
    """The Lovasz extension of the Jaccard loss evaluated as a set function on every prefix (O(N^2)) -> L_c (C,)."""
    err, valid = np.asarray(err, np.float64), np.asarray(valid, bool)
    fg = np.asarray(fg, bool) & valid[None]
    out = np.zeros(err.shape[0])
    idx = np.flatnonzero(valid)
    for c in range(err.shape[0]):
        gt = set(int(i) for i in idx[fg[c, idx]])
        if not gt:
            continue
        order = idx[np.argsort(-err[c, idx], kind="stable")]

        def jaccard_loss(mis):
            """The set `mis` of mispredicted voxels: foreground in it is missed, background in it is a false positive."""
            missed = len(gt & mis)
            return 1.0 - (len(gt) - missed) / (len(gt) + len(mis - gt))

        prev, total = 0.0, 0.0
        for k in range(len(order)):
            cur = jaccard_loss(set(int(i) for i in order[:k + 1]))
            total += err[c, order[k]] * (cur - prev)
            prev = cur
        out[c] = total
    return out


# -------------------------------------------------------------------------------------------------------------- cases
def error_case(kind, C, N, seed=0):
    """-> (err (C, N) float32, fg (C, N) uint8, valid (N,) uint8).  kind: "random" or "ties" (errors in quarters)."""
    rng = np.random.default_rng(1000 * C + N + seed)
    y = rng.integers(0, C, N)
    valid = rng.random(N) > 0.15
    fg = (y[None] == np.arange(C)[:, None]) & valid[None]
    err = rng.random((C, N), dtype=np.float32)
    if kind == "ties":
        err = (np.floor(err * 5.0) / 4.0).clip(0.0, 1.0).astype(np.float32)
    return err, fg.astype(np.uint8), valid.astype(np.uint8)


GRID, BATCH, CLASSES = (16, 16, 8), 2, 5


@functools.lru_cache(maxsize=None)
def logit_case(name="soft"):
    """-> (logits (B, C, X, Y, Z) float32, target (B, X, Y, Z) uint8 with every class and some 255)."""
    rng = np.random.default_rng(7)
    z = (rng.standard_normal((BATCH, CLASSES) + GRID) * 2.0).astype(np.float32)
    y = rng.integers(0, CLASSES, (BATCH,) + GRID).astype(np.uint8)
    y[rng.random(y.shape) < 0.1] = 255
    if name == "saturated":
        z = np.where(rng.random(z.shape) < 0.5, 40.0, -40.0).astype(np.float32)
        z[:, 0] = np.where(rng.random(z[:, 0].shape) < 0.5, 80.0, z[:, 0])       # some voxels with one class far ahead
    assert set(range(CLASSES)) <= set(y.reshape(-1).tolist()) and (y == 255).any()
    return torch.from_numpy(z), torch.from_numpy(y)


@functools.lru_cache(maxsize=None)
def expected(name="soft"):
    """(restatement's loss, L_c, gradient) and the errors of the float32 torch formulation on the same inputs (CPU), once."""
    from occdepth_amd.loss import lovasz_loss as ll
    z, y = logit_case(name)
    r_loss, r_lc, r_grad = ll.lovasz_ref(z.numpy(), y.numpy())
    leaf = z.clone().requires_grad_(True)
    loss = ll.lovasz_softmax_torch(leaf, y)
    loss.backward()
    errs = dict(loss=abs(float(loss.detach()) - r_loss), grad=np.abs(leaf.grad.numpy() - r_grad).max() / np.abs(r_grad).max())
    return dict(loss=r_loss, lc=r_lc, grad=r_grad), errs


# --------------------------------------------------------------------------------------------------------------- ABI
def test_exports_and_abi_version(hip_lib):
    from occdepth_amd import hip
    for name in ("occd_sort_pairs_u32", "occd_lovasz_errors", "occd_lovasz_ranks", "occd_lovasz_bwd"):
        assert name in hip.EXPORTS
        assert getattr(hip_lib, name) is not None                       # the cross-compiled library exports it
    assert hip.ABI_VERSION == 22 and hip_lib.occd_abi_version() == 22
    assert hip.SORT_TILE >= 256 and hip.SORT_TILE % 256 == 0 and hip.SORT_RADIX_BITS in (8, 11)
    assert hip.LOVASZ_INVALID_KEY > ONE_BITS and hip.LOVASZ_INVALID_KEY < 1 << hip.LOVASZ_KEY_BITS and hip.LOVASZ_Q == Q


def test_library_validates_arguments_before_any_launch(hip_lib):
    """OCCD_EINVAL (-1) for what the header names, with no GPU in the machine."""
    from occdepth_amd import hip
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    ptr += (-ptr) % 16

    def sort_args(**kw):
        a = hip.SortArgs()
        a.keys = a.vals = a.keys_alt = a.vals_alt = a.hist = ptr
        a.n, a.segments, a.begin_bit, a.end_bit = 8, 1, 0, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert hip_lib.occd_sort_pairs_u32(None, None) == -1
    for kw in (dict(keys=None), dict(vals=None), dict(keys_alt=None), dict(vals_alt=None), dict(hist=None), dict(n=0),
               dict(n=1 << 31), dict(segments=0), dict(segments=65536), dict(segments=1024, n=1 << 30), dict(begin_bit=-1),
               dict(begin_bit=8, end_bit=8), dict(end_bit=33)):
        assert hip_lib.occd_sort_pairs_u32(sort_args(**kw), None) == -1, kw

    def args(**kw):
        a = hip.LovaszArgs()
        for f in ("logits", "target", "keys", "vals", "tsum", "q", "fg_count", "loss_q", "gscale", "grad"):
            setattr(a, f, ptr)
        a.batch, a.S, a.C, a.c0, a.cc, a.ignore = 1, 8, 5, 0, 5, 255
        a.s_b, a.s_c, a.s_v = 40, 8, 1
        a.g_b, a.g_c, a.g_v, a.g_pad = 40, 8, 1, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    volume = [dict(batch=0), dict(S=0), dict(S=1 << 31), dict(batch=2, S=1 << 30), dict(C=1), dict(C=33), dict(c0=-1), dict(cc=0),
              dict(c0=3, cc=3)]
    logits = [dict(logits=None), dict(target=None), dict(s_c=1, s_v=6), dict(s_c=1, s_v=8, s_b=41), dict(s_v=0)]
    for fn in (hip_lib.occd_lovasz_errors, hip_lib.occd_lovasz_ranks, hip_lib.occd_lovasz_bwd):
        assert fn(None, None) == -1 and fn(ctypes.byref(hip.LovaszArgs()), None) == -1
        for kw in volume:
            assert fn(args(**kw), None) == -1, kw
    for kw in logits + [dict(keys=None), dict(vals=None)]:
        assert hip_lib.occd_lovasz_errors(args(**kw), None) == -1, kw
    for kw in (dict(keys=None), dict(vals=None), dict(tsum=None), dict(q=None), dict(fg_count=None), dict(loss_q=None)):
        assert hip_lib.occd_lovasz_ranks(args(**kw), None) == -1, kw
    for kw in logits + [dict(q=None), dict(gscale=None), dict(grad=None), dict(g_pad=8), dict(g_c=1, g_v=8, g_pad=4),
                        dict(g_c=1, g_v=8, g_pad=12), dict(g_c=1, g_v=8, g_pad=6)]:
        assert hip_lib.occd_lovasz_bwd(args(**kw), None) == -1, kw


# ------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("kind", ["random", "ties"])
def test_restatement_equals_brute_force(kind):
    from occdepth_amd.loss.lovasz_loss import lovasz_ref_from_errors
    err, fg, valid = error_case(kind, 3, 41)
    lc, _ = lovasz_ref_from_errors(err, fg.astype(bool), valid.astype(bool))
    want = brute_force(err, fg, valid)
    assert want.min() > 0 and np.abs(lc - want).max() <= 1e-13


@pytest.mark.parametrize("kind", ["random", "ties"])
@pytest.mark.parametrize("C,N", [(2, 1), (3, 41), (5, 3000)])
def test_closed_form_equals_the_cumsum_differences(kind, C, N):
    from occdepth_amd import hip
    from occdepth_amd.loss.lovasz_loss import lovasz_ref_from_errors
    err, fg, valid = error_case(kind, C, N)
    q, loss_q, G = closed_form(err, fg, valid)
    lc, g = lovasz_ref_from_errors(err, fg.astype(bool), valid.astype(bool))
    signed = np.where(fg.astype(bool), -g, g)
    # g is at most 1: the cumsum differences carry an absolute error of a unit of the wide float, q one float32 rounding
    assert np.abs(q - signed).max() <= 2.0 ** -24 * np.abs(signed).max() + 1e-15
    assert np.abs(loss_q / 2.0 ** Q - lc).max() <= hip.lovasz_value_bound(N) + N * float(np.finfo(np.longdouble).eps)
    assert (G == (fg.astype(bool) & valid.astype(bool)[None]).sum(1)).all()
    if kind == "ties" and N > 1000:
        assert len(np.unique(err)) <= 5                         # masses of ties


# --------------------------------------------------------------------------------------------------- torch formulation
def test_torch_formulation_agrees_with_the_restatement():
    from occdepth_amd.loss import lovasz_loss as ll
    z, y = logit_case()
    z = z[:, :, :8, :8, :4].double().clone().requires_grad_(True)
    y = y[:, :8, :8, :4]
    loss = ll.lovasz_softmax_torch(z, y)
    loss.backward()
    r_loss, r_lc, r_grad = ll.lovasz_ref(z.detach().numpy(), y.numpy())
    assert r_loss > 0.1 and abs(float(loss.detach()) - r_loss) <= 1e-12
    assert np.abs(z.grad.numpy() - r_grad).max() <= 1e-12 and np.abs(r_grad).max() > 1e-5
    # a long target is the same target
    assert torch.equal(ll.lovasz_softmax_torch(z.detach(), y.long()), loss.detach())


def test_gradcheck_away_from_ties():
    from occdepth_amd.loss.lovasz_loss import lovasz_softmax_torch
    g = torch.Generator().manual_seed(5)
    z = (torch.randn((1, 3, 2, 3, 2), generator=g, dtype=torch.float64) * 1.5).requires_grad_(True)
    y = torch.tensor([0, 1, 2, 1, 0, 2, 255, 1, 0, 2, 1, 0], dtype=torch.uint8).reshape(1, 2, 3, 2)
    p = torch.softmax(z.detach(), 1).permute(0, 2, 3, 4, 1).reshape(-1, 3)
    onehot = torch.nn.functional.one_hot(y.reshape(-1).long().clamp(max=2), 3).double()
    e = (onehot - p).abs()[y.reshape(-1) != 255]
    for c in range(3):                                           # piecewise linear in p: stay inside one piece
        s = e[:, c].sort().values
        assert float((s[1:] - s[:-1]).min()) > 1e-3
    assert torch.autograd.gradcheck(lambda t: lovasz_softmax_torch(t, y), (z,), eps=1e-6, atol=1e-7)


def test_edge_cases_of_the_torch_path():
    from occdepth_amd.loss.lovasz_loss import LovaszSoftmaxLoss, lovasz_ref
    fn = LovaszSoftmaxLoss()
    g = torch.Generator().manual_seed(9)
    z = torch.randn((1, 4, 3, 3, 2), generator=g, dtype=torch.float64).requires_grad_(True)
    unknown = torch.full((1, 3, 3, 2), 255, dtype=torch.uint8)
    loss = fn(z, unknown)                                                        # all unknown: 0 and a zero gradient
    loss.backward()
    assert float(loss.detach()) == 0.0 and not z.grad.any() and torch.isfinite(z.grad).all()
    y = torch.randint(0, 2, (1, 3, 3, 2), generator=g).to(torch.uint8)           # classes 2 and 3 are absent
    z.grad = None
    loss = fn(z, y)
    loss.backward()
    r_loss, r_lc, r_grad = lovasz_ref(z.detach().numpy(), y.numpy())
    assert r_lc[2] == 0 and r_lc[3] == 0 and abs(r_loss - r_lc[:2].sum() / 2) < 1e-15
    assert abs(float(loss.detach()) - r_loss) <= 1e-12 and np.abs(z.grad.numpy() - r_grad).max() <= 1e-12
    one = torch.full((1, 3, 3, 2), 3, dtype=torch.uint8)                          # one present class
    r_loss, r_lc, _ = lovasz_ref(z.detach().numpy(), one.numpy())
    assert abs(float(fn(z, one)) - r_loss) <= 1e-12 and (r_lc[:3] == 0).all() and abs(r_loss - r_lc[3]) < 1e-15
    z1 = torch.tensor([0.5, -0.25, 1.0], dtype=torch.float64).reshape(1, 3, 1, 1, 1)                        # N = 1
    y1 = torch.tensor([1], dtype=torch.uint8).reshape(1, 1, 1, 1)
    want = 1.0 - float(torch.softmax(z1.reshape(-1), 0)[1])                       # J of the one-element prefix is 1
    assert abs(float(fn(z1, y1)) - want) <= 1e-15
    with pytest.raises(ValueError, match="target"):
        fn(z, y[:, :2])


# ---------------------------------------------------------------------------------------------------------- host logic
def test_environment_switch_and_enable(monkeypatch):
    from test_oracle_vs_golden import build_product
    monkeypatch.delenv("OCCDEPTH_LOVASZ", raising=False)
    monkeypatch.delitem(sys.modules, "occdepth_amd.loss.lovasz_loss", raising=False)
    m, _, _ = build_product("kitti_small")
    assert m.lovasz_loss is None
    assert "occdepth_amd.loss.lovasz_loss" not in sys.modules                   # off: nothing is imported
    monkeypatch.setenv("OCCDEPTH_LOVASZ", "0")
    assert build_product("kitti_small")[0].lovasz_loss is None
    monkeypatch.setenv("OCCDEPTH_LOVASZ", "0.25")
    m, _, _ = build_product("kitti_small")
    assert m.lovasz_loss["weight"] == 0.25 and m.lovasz_loss["fn"].class_chunk is None
    assert "occdepth_amd.loss.lovasz_loss" in sys.modules
    for bad in ("much", "1,2", "-1", "nan"):
        monkeypatch.setenv("OCCDEPTH_LOVASZ", bad)
        with pytest.raises(ValueError, match="OCCDEPTH_LOVASZ|weight must be > 0"):
            build_product("kitti_small")
    monkeypatch.setenv("OCCDEPTH_LOVASZ", "x")
    with pytest.raises(ValueError, match="OCCDEPTH_LOVASZ is <weight>, got 'x'"):
        build_product("kitti_small")
    monkeypatch.delenv("OCCDEPTH_LOVASZ")
    m, _, _ = build_product("kitti_small")
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="weight must be > 0"):
            m.enable_lovasz_loss(weight=bad)
    assert m.lovasz_loss is None
    assert m.enable_lovasz_loss(weight=2, class_chunk=4) is m and m.lovasz_loss["fn"].class_chunk == 4
    with pytest.raises(ValueError, match="class_chunk"):
        m.enable_lovasz_loss(class_chunk=0)


def test_voxel_limit_and_scratch_size():
    from occdepth_amd import hip
    from occdepth_amd.loss.lovasz_loss import LovaszSoftmaxLoss
    assert hip.lovasz_check_voxels((1 << 31) - 1) == (1 << 31) - 1
    for n in (0, 1 << 31, 1 << 33):
        with pytest.raises(ValueError, match="2\\^31"):
            hip.lovasz_check_voxels(n)
    z = torch.zeros(1).expand(1, 2, 1 << 16, 1 << 15, 1)                          # 2^31 voxels, no memory behind them
    with pytest.raises(ValueError, match="2\\^31"):
        LovaszSoftmaxLoss()(z, torch.zeros(1, dtype=torch.uint8).expand(1, 1 << 16, 1 << 15, 1))
    # the flagship: 256 x 256 x 32 voxels, 20 classes, B = 1
    n, T, R = 256 * 256 * 32, hip.SORT_TILE, hip.LOVASZ_RANK_TILE
    pairs = 2 * 2 * 4 * 20 * n
    assert hip.lovasz_scratch_bytes(n, 20) == pairs + 4 * 20 * 256 * (n // T) + 4 * 20 * (n // R)
    assert hip.lovasz_scratch_bytes(n, 20, 5) == pairs // 4 + 4 * 5 * 256 * (n // T) + 4 * 5 * (n // R)
    assert hip.lovasz_scratch_bytes(T + 1, 3) == 16 * 3 * (T + 1) + 4 * 3 * 256 * 2 + 4 * 3 * (T // R + 1)
    for bad in (0, 21):
        with pytest.raises(ValueError, match="class_chunk"):
            hip.lovasz_scratch_bytes(n, 20, bad)
    assert hip.sort_passes(0, 32) == 4 and hip.sort_passes(0, 31) == 4 and hip.sort_passes(3, 11) == 1 and hip.sort_passes(0, 9) == 2
    with pytest.raises(ValueError, match="bit range"):
        hip.sort_passes(8, 8)
    assert hip.lovasz_value_bound(1 << 21) == 2.0 ** -40 + 2.0 ** -50
    assert not hip.lovasz_usable(torch.zeros(1, 5, 2, 2, 2)) and not hip.lovasz_usable(torch.zeros(1, 5, 2, 2, 2).double())
    with pytest.raises(RuntimeError, match="GPU"):
        hip.lovasz_errors(torch.zeros(1, 5, 2, 2, 2), torch.zeros(1, 2, 2, 2, dtype=torch.uint8), 0, 5,
                          torch.zeros(5, 8, dtype=torch.int32), torch.zeros(5, 8, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="int32"):
        hip.sort_pairs(torch.zeros(1, 4), torch.zeros(1, 4))
