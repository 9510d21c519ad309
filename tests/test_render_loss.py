"""Depth-rendering loss (K36), without a GPU: a restatement of include/occdepth_amd.h's K36 section -- per ray a scalar
float32 walk (numpy float32 scalars round once per operation, like the kernel's contract-off arithmetic) and a float64
compositing loop -- checked against finite differences, and the package's torch formulation, view algebra, model hook and
argument validation checked against it.  tests/test_render_loss_gpu.py holds the kernels to the same restatement."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

F = np.float32
REL_FLOOR = 0.25


# ------------------------------------------------------------------------------------------------- the restatement
def walk_ref(view, dims, u, v, max_depth):
    """One ray of pixel (u, v): -> (alive, t_entry, t_end, [(voxel, t), ...]) in float32, the walk of the header."""
    X, Y, Z = dims
    g = [F(x) for x in view]
    md = F(max_depth)
    inf = F(np.inf)
    with np.errstate(all="ignore"):
        fu, fv = F(u) + F(0.5), F(v) + F(0.5)
        o = [g[i] + fu * g[3 + i] + fv * g[6 + i] for i in range(3)]
        d = [g[9 + i] + fu * g[12 + i] + fv * g[15 + i] for i in range(3)]
        alive = all(np.isfinite(c) for c in o + d)
        tn, tf = -inf, inf
        inv = [F(1) / d[i] if d[i] != 0 else F(0) for i in range(3)]
        ext = [F(X), F(Y), F(Z)]
        for i in range(3):
            if d[i] != 0:
                a, c = (F(0) - o[i]) * inv[i], (ext[i] - o[i]) * inv[i]
                if min(a, c) > tn:
                    tn = min(a, c)
                tf = min(tf, max(a, c))
            elif not (o[i] >= 0 and o[i] < ext[i]):
                alive = False
        t = tn if tn > 0 else F(0)
        if not tf >= t:
            alive = False
        t_end = min(tf, md) if alive else md
        t_entry = t
        steps = []
        if alive and t < md:
            idx = [int(min(max(np.floor(o[i] + d[i] * t), F(0)), ext[i] - F(1))) for i in range(3)]
            sg = [1 if d[i] > 0 else -1 if d[i] < 0 else 0 for i in range(3)]
            edge = lambda i: (F(idx[i] + (sg[i] > 0)) - o[i]) * inv[i] if sg[i] else inf
            m = [edge(i) for i in range(3)]
            for _ in range(X + Y + Z + 3):
                steps.append(((idx[0] * Y + idx[1]) * Z + idx[2], t))
                ax = 0 if (m[0] <= m[1] and m[0] <= m[2]) else 1 if m[1] <= m[2] else 2
                if not m[ax] < md:
                    break
                nxt = m[ax]
                idx[ax] += sg[ax]
                if idx[ax] < 0 or idx[ax] >= dims[ax]:
                    break
                m[ax] = edge(ax)
                t = nxt
    return alive, t_entry, t_end, steps


def softmax_ref(logits):
    """(B, C, ...) -> float64 probabilities (B, C, S) and the opacity sum_{c > 0} p_c (B, S)."""
    z = np.asarray(logits, dtype=np.float64).reshape(logits.shape[0], logits.shape[1], -1)
    e = np.exp(z - z.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    return p, p[:, 1:].sum(1)


class Reference:
    """Everything about one (logits, views, D, max_depth) at full resolution: every pixel's ray is walked once."""

    def __init__(self, logits, views, D, max_depth, rays_of=None):
        self.logits = np.asarray(logits, dtype=np.float64)
        B, C = self.logits.shape[:2]
        self.dims = tuple(self.logits.shape[2:])
        self.p, self.a = softmax_ref(self.logits)
        self.D = np.asarray(D, dtype=np.float32).reshape(B, *D.shape[-2:])
        self.H, self.W = self.D.shape[1:]
        self.max_depth = float(max_depth)
        if rays_of is None:
            rays_of = lambda b, v, u: walk_ref(views[b], self.dims, u, v, max_depth)
        self.rays = [[[rays_of(b, v, u) for u in range(self.W)] for v in range(self.H)] for b in range(B)]
        self.depth = np.zeros((B, self.H, self.W))
        self.alpha = np.zeros((B, self.H, self.W))
        self.valid = np.zeros((B, self.H, self.W), dtype=bool)
        self.Dr = np.zeros((B, self.H, self.W))
        self.kind = np.empty((B, self.H, self.W), dtype=object)
        for b in range(B):
            for v in range(self.H):
                for u in range(self.W):
                    alive, t_entry, t_end, steps = self.rays[b][v][u]
                    T, acc = 1.0, 0.0
                    for vox, t in steps:
                        a = self.a[b, vox]
                        acc += T * a * float(t)
                        T *= 1.0 - a
                    self.depth[b, v, u] = acc + T * float(t_end)
                    self.alpha[b, v, u] = 1.0 - T
                    d = self.D[b, v, u]
                    kind = ("miss" if not alive else "nan" if not np.isfinite(d) else "zero" if d == 0 else
                            "negative" if d < 0 else "far" if d > F(max_depth) else "front" if not d > t_entry else
                            "behind" if d > t_end else "inside")
                    self.kind[b, v, u] = kind
                    self.valid[b, v, u] = kind in ("behind", "inside")
                    self.Dr[b, v, u] = min(float(d), float(t_end)) if self.valid[b, v, u] else 0.0

    def pixels(self, stride, offset):
        return [(b, v, u) for b in range(self.D.shape[0]) for v in range(offset[1], self.H, stride)
                for u in range(offset[0], self.W, stride)]

    def images(self, stride=1, offset=(0, 0)):
        sl = (slice(None), slice(offset[1], None, stride), slice(offset[0], None, stride))
        return self.depth[sl], self.alpha[sl], self.valid[sl], self.Dr[sl]

    def omega(self, Dr, norm):
        return 1.0 if norm == "abs" else 1.0 / max(Dr, REL_FLOOR)

    def loss(self, stride=1, offset=(0, 0), norm="abs"):
        """-> (L, #valid rays)."""
        total, n = 0.0, 0
        for b, v, u in self.pixels(stride, offset):
            if self.valid[b, v, u]:
                total += self.omega(self.Dr[b, v, u], norm) * abs(self.depth[b, v, u] - self.Dr[b, v, u])
                n += 1
        return total / max(1, n), n

    def grad_opacity(self, stride=1, offset=(0, 0), norm="abs"):
        """d L / d a (B, S) by the REVERSE recursion R_{k-1} = a_k t_k + (1 - a_k) R_k, d d^ / d a_k = T_k (t_k - R_k)."""
        n = max(1, self.loss(stride, offset, norm)[1])
        ga = np.zeros_like(self.a)
        for b, v, u in self.pixels(stride, offset):
            if not self.valid[b, v, u]:
                continue
            _, _, t_end, steps = self.rays[b][v][u]
            Dr = self.Dr[b, v, u]
            s = np.sign(self.depth[b, v, u] - Dr) * self.omega(Dr, norm) / n
            Ts, T = [], 1.0
            for vox, t in steps:
                Ts.append(T)
                T *= 1.0 - self.a[b, vox]
            R = float(t_end)
            for k in range(len(steps) - 1, -1, -1):
                vox, t = steps[k]
                ga[b, vox] += s * Ts[k] * (float(t) - R)
                R = self.a[b, vox] * float(t) + (1.0 - self.a[b, vox]) * R
        return ga

    def grad_logits(self, stride=1, offset=(0, 0), norm="abs"):
        """d L / d z: d a / d z_c = p_c ([c > 0] - a)."""
        ga = self.grad_opacity(stride, offset, norm)
        pos = np.ones(self.p.shape[1])
        pos[0] = 0.0
        g = ga[:, None, :] * self.p * (pos[None, :, None] - self.a[:, None, :])
        return g.reshape(self.logits.shape)


# ------------------------------------------------------------------------------------------------------- the cases
R_CAM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])     # camera z = world x, x = -world y, y = -world z
VOXEL = 0.2


def perspective_view(dims, centre, focal, image_hw, yaw=0.0, flip=False):
    """A pinhole camera at `centre` (metres; the grid is centred on the x axis: origin (0, -Y/2, -Z/2) voxels) looking along
    +x turned by `yaw` -> (18,) float32, through render.camera_view."""
    from occdepth_amd import render
    H, W = image_hw
    k = torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, H / 2.0], [0.0, 0.0, 1.0]], dtype=torch.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    R = R_CAM @ np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    E = np.eye(4)
    E[:3, :3] = R
    E[:3, 3] = -R @ np.asarray(centre, dtype=np.float64)
    origin = (0.0, -VOXEL * dims[1] / 2.0, -VOXEL * dims[2] / 2.0)
    return render.camera_view(k, torch.from_numpy(E), origin, VOXEL, flip=flip, width=W if flip else None)


def soft_logits(rng, B, C, dims):
    """Random logits whose opacities span 1e-4 .. 1 - 1e-4: the empty class' logit is uniform over +-11."""
    z = rng.standard_normal((B, C) + tuple(dims))
    z[:, 0] = rng.uniform(-11.0, 11.0, (B,) + tuple(dims))
    return z.astype(np.float32)


def depth_map(rng, rays_of, B, image_hw, max_depth):
    """D with every kind of pixel: no measurement, NaN, negative, past max_depth, in front of the grid's entry, behind its
    exit, and inside.  rays_of(b, v, u) -> (alive, t_entry, t_end, steps)."""
    H, W = image_hw
    D = np.zeros((B, H, W), dtype=np.float32)
    for b in range(B):
        for v in range(H):
            for u in range(W):
                alive, t0, t1, _ = rays_of(b, v, u)
                r = rng.uniform()
                lo, hi = float(t0), float(t1)
                if r < 0.12:
                    D[b, v, u] = 0.0
                elif r < 0.15:
                    D[b, v, u] = np.nan if rng.uniform() < 0.5 else np.inf
                elif r < 0.18:
                    D[b, v, u] = -1.0
                elif r < 0.24:
                    D[b, v, u] = max_depth * (1.0 + rng.uniform(0.01, 0.5))
                elif r < 0.32:
                    D[b, v, u] = lo * rng.uniform(0.2, 0.99)                   # 0 when the camera is inside: no measurement
                elif r < 0.44:
                    D[b, v, u] = hi + (max_depth - hi) * rng.uniform(0.05, 1.0)    # behind the exit, within max_depth
                else:
                    D[b, v, u] = lo + (hi - lo) * rng.uniform(0.02, 0.98) if hi > lo else hi
    return D


CASES = {
    # name: dims, image (H, W), max_depth, views
    "small": dict(dims=(16, 12, 8), image=(13, 21), max_depth=6.0, seed=11,
                  views=lambda d, hw: [perspective_view(d, (0.33, 0.11, 0.07), 9.0, hw, yaw=0.3), "bev"]),
    "large": dict(dims=(24, 20, 12), image=(37, 122), max_depth=3.5, seed=12,
                  views=lambda d, hw: [perspective_view(d, (-1.03, 1.71, 0.21), 60.0, hw),
                                       perspective_view(d, (0.41, -0.52, -0.13), 45.0, hw, yaw=-0.2)]),
}
B, C = 2, 5


def case_views(name):
    from occdepth_amd import render
    c = CASES[name]
    vs = [render.bev_view(c["dims"], 1, device="cpu") if isinstance(v, str) else v for v in c["views"](c["dims"], c["image"])]
    return torch.stack([v.reshape(18).float() for v in vs])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (logits (B, C, X, Y, Z) f32, views (B, 18) f32, D (B, 1, H, W) f32, max_depth, Reference), built once."""
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    logits = soft_logits(rng, B, C, c["dims"])
    views = case_views(name)
    vn = views.numpy()
    cache = {}

    def rays_of(b, v, u):
        if (b, v, u) not in cache:
            cache[(b, v, u)] = walk_ref(vn[b], c["dims"], u, v, c["max_depth"])
        return cache[(b, v, u)]

    D = depth_map(rng, rays_of, B, c["image"], c["max_depth"])
    ref = Reference(logits, vn, D, c["max_depth"], rays_of)
    return torch.from_numpy(logits), views, torch.from_numpy(D)[:, None], c["max_depth"], ref


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


STRIDES = [(1, (0, 0)), (3, (1, 2))]


# ------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_hold_every_kind_of_ray(name):
    """The inputs the GPU tests run on contain valid and invalid rays of each kind, at both strides; opacities span
    1e-4 .. 1 - 1e-4; no valid ray has d^ == D_r (the sign in the gradient is never the sign of zero)."""
    _, _, _, max_depth, ref = case(name)
    assert ref.a.min() < 1e-4 and ref.a.max() > 1 - 1e-4
    # every kind in the full image; the few rays of a strided pass still hold missing, unmeasured and both valid kinds
    want = {1: {"miss", "zero", "nan", "negative", "far", "front", "behind", "inside"}, 3: {"miss", "zero", "behind", "inside"}}
    for stride, offset in STRIDES:
        kinds = {ref.kind[p] for p in ref.pixels(stride, offset)}
        assert want[stride] <= kinds, (name, stride, sorted(want[stride] - kinds))
    assert not np.any(ref.valid & (ref.depth == ref.Dr))
    cut = sum(1 for b in range(B) for v in range(ref.H) for u in range(ref.W)
              if ref.rays[b][v][u][0] and float(ref.rays[b][v][u][2]) == max_depth)
    assert cut > 0                                                     # max_depth cuts some rays short
    dirs = np.asarray(case_views(name))[:, 9:]
    if name == "small":
        assert np.count_nonzero(dirs[1, :3]) == 1 and not dirs[1, 3:].any()        # orthographic: two zero components


def test_restatement_gradient_agrees_with_finite_differences():
    rng = np.random.default_rng(5)
    dims, hw, max_depth = (8, 6, 4), (3, 4), 1.4
    logits = soft_logits(rng, 1, 3, dims).astype(np.float64)
    logits[:, 0] = rng.uniform(-3.0, 3.0, (1,) + dims)                 # every voxel carries a gradient that is not tiny
    view = perspective_view(dims, (0.13, 0.05, 0.02), 3.0, hw, yaw=0.2).numpy()[None]
    probe = Reference(logits, view, np.zeros((1,) + hw, dtype=np.float32), max_depth)
    D = depth_map(rng, lambda b, v, u: probe.rays[b][v][u], 1, hw, max_depth)
    D[0, 0, :] = [0.4, 0.9, 1.2, 0.7]                                  # a handful of rays with a measurement inside
    for norm in ("abs", "rel"):
        ref = Reference(logits, view, D, max_depth)
        assert ref.valid.sum() >= 4
        g = ref.grad_logits(norm=norm)
        touched = np.argwhere(np.abs(g) > 0)
        assert len(touched) > 20
        worst = 0.0
        for i in touched[:: max(1, len(touched) // 40)]:
            h = 1e-5
            zp, zm = logits.copy(), logits.copy()
            zp[tuple(i)] += h
            zm[tuple(i)] -= h
            fd = (Reference(zp, view, D, max_depth).loss(norm=norm)[0] - Reference(zm, view, D, max_depth).loss(norm=norm)[0]) / (2 * h)
            worst = max(worst, abs(fd - g[tuple(i)]))
        # central differences: truncation h^2 f''' / 6 ~ 1e-10, rounding eps L / h ~ 1e-11, against gradients of ~1e-2
        assert worst <= 1e-8 * max(1.0, np.abs(g).max()), (norm, worst, np.abs(g).max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_float64_fallback_equals_the_restatement(name):
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, ref = case(name)
    for stride, offset in STRIDES:
        for norm in ("abs", "rel"):
            z = logits.double().requires_grad_(True)
            fn = rl.RenderDepthLoss(stride=stride, max_depth=max_depth, norm=norm, offset=offset)
            loss = fn(z, D, views)
            loss.backward()
            depth, alpha, n_valid = fn.last
            r_depth, r_alpha, r_valid, _ = ref.images(stride, offset)
            r_loss, r_n = ref.loss(stride, offset, norm)
            assert int(n_valid) == r_n == int(r_valid.sum()) and r_n > 0
            assert rel_err(depth.numpy(), r_depth) <= 1e-10 and rel_err(alpha.numpy(), r_alpha) <= 1e-10
            assert abs(float(loss.detach()) - r_loss) <= 1e-10 * abs(r_loss)
            assert rel_err(z.grad.numpy(), ref.grad_logits(stride, offset, norm)) <= 1e-10
    d, a = rl.render_depth(logits.double(), views, D.shape[-2:], max_depth=max_depth)
    assert rel_err(d.numpy(), ref.depth) <= 1e-10 and rel_err(a.numpy(), ref.alpha) <= 1e-10


@pytest.mark.parametrize("name", sorted(CASES))
def test_strided_rays_are_rows_and_columns_of_the_full_image(name):
    """Ray (i, j) at stride s and offset (ou, ov) IS pixel (ou + s i, ov + s j): bit-equal d^ and opacity."""
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, _ = case(name)
    full_d, full_a = rl.render_depth(logits, views, D.shape[-2:], max_depth=max_depth)
    for stride, offset in [(3, (1, 2)), (2, (0, 1)), (4, (3, 0))]:
        d, a = rl.render_depth(logits, views, D.shape[-2:], stride=stride, offset=offset, max_depth=max_depth)
        assert torch.equal(d, full_d[:, offset[1]::stride, offset[0]::stride])
        assert torch.equal(a, full_a[:, offset[1]::stride, offset[0]::stride])
        walk = rl.walk_rays(views, logits.shape[2:], D.shape[-2:], stride, offset, max_depth)
        assert walk["shape"] == tuple(d.shape)


def test_torch_walk_is_the_restated_walk():
    """The vectorised float32 walk of the fallback visits the restatement's voxels at the restatement's depths, bit for bit."""
    from occdepth_amd.loss import render_loss as rl
    logits, views, D, max_depth, ref = case("small")
    walk = rl.walk_rays(views, logits.shape[2:], D.shape[-2:], 1, (0, 0), max_depth)
    S = int(np.prod(logits.shape[2:]))
    n = 0
    for b in range(B):
        for v in range(ref.H):
            for u in range(ref.W):
                alive, t_entry, t_end, steps = ref.rays[b][v][u]
                on = walk["step"][n]
                assert bool(walk["alive"][n]) == alive and int(on.sum()) == len(steps)
                assert walk["t_end"][n].item() == float(t_end)
                assert [int(i) - b * S for i in walk["index"][n][on]] == [s[0] for s in steps]
                assert [float(t) for t in walk["t"][n][on]] == [float(s[1]) for s in steps]
                n += 1


def test_mirrored_view_mirrors_the_rays():
    from occdepth_amd.loss import render_loss as rl
    from occdepth_amd import render
    dims, hw = (16, 12, 8), (13, 21)
    k = torch.tensor([[9.0, 0.0, 10.5], [0.0, 9.0, 6.5], [0.0, 0.0, 1.0]], dtype=torch.float64)[None].expand(2, 3, 3)
    E = torch.eye(4, dtype=torch.float64)
    E[:3, :3] = torch.from_numpy(R_CAM)
    E[:3, 3] = torch.from_numpy(-R_CAM @ np.array([0.33, 0.11, 0.07]))
    E = E[None].expand(2, 4, 4)
    origin = (0.0, -1.2, -0.8)
    views = rl.frame_views(k, E, origin, VOXEL, width=hw[1], flip=torch.tensor([False, True]))
    assert torch.equal(views[0], render.camera_view(k[0], E[0], origin, VOXEL))
    assert torch.equal(views[1], render.camera_view(k[0], E[0], origin, VOXEL, flip=True, width=hw[1]))
    z = torch.from_numpy(soft_logits(np.random.default_rng(3), 1, 3, dims)).double().expand(2, 3, *dims)
    d, _ = rl.render_depth(z, views, hw, max_depth=4.0)
    # The float32 ray directions of the mirrored view differ from the plain ones in the last bits.  d^ is continuous in the
    # direction except where a ray grazes a voxel corner (there is no path-length weighting: a clipped corner counts like a
    # full crossing), so nearly every ray agrees to float32 accuracy and a grazing ray may differ by a visible amount.
    diff = (d[1].flip(-1) - d[0]).abs() / d[0].abs().max()
    assert float((diff <= 1e-6).double().mean()) >= 0.95 and float(diff.median()) <= 1e-6


# ------------------------------------------------------------------------------------------------------ model hook
class _Stub:
    """The attributes OccDepth's render-loss hook touches, without the networks."""
    RENDER_VOXEL_METRES = {"kitti": 0.2, "NYU": 0.08}

    def __init__(self, dataset="kitti"):
        from occdepth_amd.models.OccDepth import OccDepth
        self.dataset, self.full_scene_size, self.logged = dataset, (16, 12, 8), {}
        self.render_loss, self._fast_train = None, "captured"
        for name in ("enable_render_loss", "_render_loss_views", "_render_loss_step", "_kitti_origin"):
            setattr(self, name, types.MethodType(getattr(OccDepth, name), self))

    def _log(self, key, value):
        self.logged[key] = value.detach()


def _stub_batch(flip=False):
    E = np.eye(4)
    E[:3, :3] = R_CAM
    E[:3, 3] = -R_CAM @ np.array([0.33, 0.11, 0.07])
    ida = torch.eye(4)[None].repeat(2, 1, 1)
    if flip:
        ida[:, 0, 0] = -1.0
    return {"cam_k": [torch.tensor([[9.0, 0.0, 10.5], [0.0, 9.0, 6.5], [0.0, 0.0, 1.0]])[None].repeat(2, 1, 1)],
            "T_velo_2_cam": [torch.from_numpy(E).float()[None].repeat(2, 1, 1)], "ida_mats": [ida],
            "vox_origin": torch.tensor([[0.0, -1.2, -0.8]])}


def test_model_hook_logic():
    from occdepth_amd.loss import render_loss as rl
    from occdepth_amd import render
    with pytest.raises(NotImplementedError, match="NYU"):
        _Stub("NYU").enable_render_loss()
    m = _Stub()
    assert m.enable_render_loss(weight=0.5, stride=2) is m and m._fast_train is None
    assert m.render_loss["weight"] == 0.5 and m.render_loss["fn"].stride == 2
    assert m.render_loss["fn"].max_depth == 54.0 and m.render_loss["fn"].norm == "abs"
    for bad in (dict(weight=0.0), dict(stride=0), dict(max_depth=200.0), dict(norm="l2")):
        with pytest.raises((ValueError, RuntimeError)):
            _Stub().enable_render_loss(**bad)
    z = torch.from_numpy(soft_logits(np.random.default_rng(4), 1, 3, (16, 12, 8)))
    D = torch.full((1, 1, 13, 21), 1.0)
    batch = _stub_batch()
    assert m._render_loss_step("train", batch, z, None) is None and not m.logged          # no depth target: nothing
    assert m._render_loss_step("train", batch, z, torch.zeros(1, 1, 0, 0)) is None and not m.logged
    assert m._render_loss_step("test", batch, z, D) is None and not m.logged
    loss = m._render_loss_step("train", batch, z, D)
    assert sorted(m.logged) == ["train/loss_render"] and torch.equal(m.logged["train/loss_render"], loss)
    k, E, origin = render.batch_camera(batch, "kitti", (0.0, -1.2, -0.8))
    views = render.camera_view(k, E, origin, VOXEL)
    want = rl.RenderDepthLoss(stride=2, max_depth=54.0)(z, D, views) * 0.5
    assert torch.equal(loss, want)
    m.logged = {}
    m._render_loss_step("val", batch, z, D)
    assert sorted(m.logged) == ["val/loss_render", "val/render_abs_rel", "val/render_rmse"]
    depth, _, _ = m.render_loss["fn"].last
    valid, target = m.render_loss["fn"].valid_rays(D, views, (16, 12, 8))
    err = (depth - target)[valid]
    assert abs(float(m.logged["val/render_rmse"]) - float((err * err).mean().sqrt())) <= 1e-6 * float(err.abs().max())
    assert abs(float(m.logged["val/render_abs_rel"]) - float((err.abs() / target[valid]).mean())) <= 1e-6
    # a mirrored frame is rendered through the mirrored view
    mirrored = m._render_loss_views(_stub_batch(flip=True), z, 21)
    assert torch.equal(mirrored, render.camera_view(k, E, origin, VOXEL, flip=True, width=21))


def test_environment_switch_parsing(monkeypatch):
    """OCCDEPTH_RENDER_LOSS=<weight>[,<stride>] as OccDepth.__init__ reads it."""
    from test_oracle_vs_golden import build_product
    monkeypatch.setenv("OCCDEPTH_RENDER_LOSS", "0.25,2")
    m, _, _ = build_product("kitti_small")
    assert m.render_loss["weight"] == 0.25 and m.render_loss["fn"].stride == 2
    monkeypatch.setenv("OCCDEPTH_RENDER_LOSS", "2")
    m, _, _ = build_product("kitti_small")
    assert m.render_loss["weight"] == 2.0 and m.render_loss["fn"].stride == 4
    monkeypatch.setenv("OCCDEPTH_RENDER_LOSS", "1,2,3")
    with pytest.raises(ValueError, match="OCCDEPTH_RENDER_LOSS"):
        build_product("kitti_small")
    monkeypatch.delenv("OCCDEPTH_RENDER_LOSS")
    m, _, _ = build_product("kitti_small")
    assert m.render_loss is None


# -------------------------------------------------------------------------------------------- argument validation
def test_wrappers_validate_arguments_without_a_gpu(hip_lib):
    from occdepth_amd import hip
    assert hip.render_loss_rays((370, 1220), 4, (0, 0)) == (93, 305)
    assert hip.render_loss_rays((13, 21), 3, (1, 2)) == (4, 7)
    for args in (((13, 21), 0, (0, 0)), ((13, 21), 3, (3, 0)), ((13, 21), 3, (0, -1)), ((0, 21), 1, (0, 0)),
                 ((2000, 2000), 1, (0, 0)), ((2, 30), 4, (0, 3))):
        with pytest.raises(RuntimeError):
            hip.render_loss_rays(*args)
    z = torch.zeros(1, 5, 4, 4, 4)
    op = torch.zeros(1, 64)
    view = torch.zeros(1, 18)
    D = torch.zeros(1, 1, 6, 8)
    assert not hip.render_loss_usable(z) and not hip.render_loss_usable(z.double())
    with pytest.raises(RuntimeError, match="float32"):
        hip.render_opacity(z.double())
    with pytest.raises(RuntimeError, match="C <= 32"):
        hip.render_opacity(torch.zeros(1, 33, 2, 2, 2))
    with pytest.raises(RuntimeError, match="C <= 32"):
        hip.render_opacity(torch.zeros(1, 1, 2, 2, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        hip.render_opacity(z)
    with pytest.raises(RuntimeError, match="opacity"):
        hip.render_depth_fwd(torch.zeros(1, 63), view, (4, 4, 4), (6, 8))
    with pytest.raises(RuntimeError, match="views"):
        hip.render_depth_fwd(op, torch.zeros(2, 18), (4, 4, 4), (6, 8))
    with pytest.raises(RuntimeError, match="max_depth"):
        hip.render_depth_fwd(op, view, (4, 4, 4), (6, 8), max_depth=129.0)
    with pytest.raises(RuntimeError, match="max_depth"):
        hip.render_depth_fwd(op, view, (4, 4, 4), (6, 8), max_depth=0.0)
    with pytest.raises(RuntimeError, match="norm"):
        hip.render_depth_fwd(op, view, (4, 4, 4), (6, 8), norm="l2")
    with pytest.raises(RuntimeError, match="gt_depth"):
        hip.render_depth_fwd(op, view, (4, 4, 4), (6, 8), gt_depth=torch.zeros(1, 1, 6, 9))
    with pytest.raises(RuntimeError, match="gt_depth"):
        hip.render_depth_fwd(op, view, (4, 4, 4), (6, 8), gt_depth=D.double())
    with pytest.raises(RuntimeError, match="GPU"):
        hip.render_depth_fwd(op, view, (4, 4, 4), (6, 8), gt_depth=D)
    with pytest.raises(RuntimeError, match="gt_depth"):
        hip.render_depth_bwd_rays(op, view, (4, 4, 4), (6, 8), 1, (0, 0), 10.0, None, "abs", torch.zeros(1, 6, 8), torch.zeros(1, 64, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="hsum"):
        hip.render_depth_bwd_voxels(z, torch.zeros(1, 64), torch.zeros(1))
    with pytest.raises(RuntimeError, match="gscale"):
        hip.render_depth_bwd_voxels(z, torch.zeros(1, 64, dtype=torch.int64), torch.zeros(2))


def test_library_validates_arguments_before_any_launch(hip_lib):
    """occd_render_*: OCCD_EINVAL (-1) for every argument the header names, with no GPU in the machine."""
    from occdepth_amd import hip
    fns = [hip_lib.occd_render_opacity, hip_lib.occd_render_depth_fwd, hip_lib.occd_render_depth_bwd_rays,
           hip_lib.occd_render_depth_bwd_voxels]
    for fn in fns:
        assert fn(None, None) == -1
        assert fn(ctypes.byref(hip.RenderLossArgs()), None) == -1
    buf = (ctypes.c_float * 64)()
    ptr = ctypes.addressof(buf)
    ptr += (-ptr) % 16

    def args(**kw):
        a = hip.RenderLossArgs()
        for f in ("logits", "opacity", "views", "gt_depth", "depth", "alpha", "stats", "hsum", "gscale", "grad"):
            setattr(a, f, ptr)
        a.batch, a.C, a.X, a.Y, a.Z = 1, 5, 2, 2, 2
        a.s_b, a.s_c, a.s_v = 40, 8, 1
        a.g_b, a.g_c, a.g_v, a.g_pad = 40, 8, 1, 0
        a.d_b, a.d_h, a.d_w = 48, 8, 1
        a.H, a.W, a.h, a.w, a.stride, a.off_u, a.off_v = 6, 8, 6, 8, 1, 0, 0
        a.max_depth, a.norm = 10.0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    opacity, fwd, rays, voxels = fns
    bad_volume = [dict(batch=0), dict(batch=257), dict(X=0), dict(X=1 << 16, Y=1 << 16), dict(Z=-1)]
    bad_logits = [dict(logits=None), dict(C=1), dict(C=33), dict(s_c=1, s_v=6), dict(s_c=1, s_v=8, s_b=41), dict(s_v=0)]
    bad_rays = [dict(views=None), dict(opacity=None), dict(depth=None), dict(H=0), dict(stride=0), dict(off_u=1), dict(off_v=-1),
                dict(h=5), dict(w=9), dict(H=2048, W=2048, h=2048, w=2048), dict(max_depth=0.0), dict(max_depth=128.5),
                dict(max_depth=float("nan")), dict(norm=2), dict(d_h=-8)]
    for kw in bad_volume + bad_logits + [dict(opacity=None)]:
        assert opacity(args(**kw), None) == -1, kw
    for kw in bad_volume + bad_rays + [dict(alpha=None), dict(stats=None), dict(gt_depth=None)]:
        assert fwd(args(**kw), None) == -1, kw
    for kw in bad_volume + bad_rays + [dict(gt_depth=None), dict(hsum=None)]:
        assert rays(args(**kw), None) == -1, kw
    for kw in bad_volume + bad_logits + [dict(hsum=None), dict(gscale=None), dict(grad=None), dict(g_pad=8), dict(g_c=1, g_v=8, g_pad=4),
                                         dict(g_c=1, g_v=8, g_pad=12), dict(g_c=1, g_v=8, g_pad=6)]:
        assert voxels(args(**kw), None) == -1, kw
    assert hip.ABI_VERSION == 22
