"""CPU: per-frame visibility (K34, occd_frame_visibility) and the weighted votes of the sequence map.

`carve_ref` restates the kernel's walk (csrc/visibility.hip on the walk of csrc/raycast.h) in numpy, in the dtype it is
given, and returns the marked volume and the hits; tests/test_visibility_gpu.py holds the kernel to its float32 run byte for
byte.  `WeightedMapRef` / `sample_ref_weighted` extend the integer restatements of tests/test_map.py and
tests/test_map_sample.py by a weight per voxel; tests/test_map_weighted_gpu.py holds the weighted entry points to them.
Here: the restatement against cast_ref and against its own float64 run, the properties that make visibility pixel-centric,
edge cases, vote_weights, the refusals, the model hook and the offline tool on kernel stand-ins, and the entry points'
argument checks before any launch."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from occdepth_amd import hip, render
from occdepth_amd import semantic_map as sm
from occdepth_amd import visibility as vis
from test_map import (B, GRIDS, HOOK_C, HOOK_DIMS, HOOK_ORIGIN, LOCAL, V, KernelStandIn, MapRef, _confusion_stand_in, _epoch,
                      _hook_steps, _hook_stub, _tool, assert_map_equals_ref, fixed_index, frames_for, generous_bricks, pose,
                      ref_coefficients, sequence, voting_labels)
from test_map_sample import SampleStandIn, sample_ref
from test_render import KITTI_VOXEL, cast_ref, kitti_calibration, kitti_origin, make_scene, rays, scene_views


# ----------------------------------------------------------------------------------------------------- the walk restated
def carve_ref(labels, origin, dirs, dtype, trace=False):
    """Every voxel a ray visits, up to and including its first occupied one (0 < label < 255) -> visible (X, Y, Z) uint8,
    hit (linear index or -1, the shape of the rays); with trace also (ray, voxel) of every visit, in walk order."""
    T = np.dtype(dtype).type
    X, Y, Z = labels.shape
    shape = origin.shape[:-1]
    o = np.ascontiguousarray(origin.reshape(-1, 3).astype(dtype))
    d = np.ascontiguousarray(dirs.reshape(-1, 3).astype(dtype))
    n = o.shape[0]
    dims = np.array([X, Y, Z], dtype=dtype)
    idims = np.array([X, Y, Z])
    flat = labels.reshape(-1).astype(np.int64)
    inf = T(np.inf)
    visible = np.zeros(X * Y * Z, dtype=np.uint8)
    visits = []
    with np.errstate(all="ignore"):
        alive = np.isfinite(o).all(1) & np.isfinite(d).all(1)
        nz = d != 0
        inv = np.where(nz, T(1) / np.where(nz, d, T(1)), T(0)).astype(dtype)
        tn, tf = np.full(n, -inf, dtype), np.full(n, inf, dtype)
        for a in range(3):                                       # slabs; a zero component is inside or outside
            ta, tc = (T(0) - o[:, a]) * inv[:, a], (dims[a] - o[:, a]) * inv[:, a]
            lo, hi = np.fmin(ta, tc), np.fmax(ta, tc)
            tn = np.where(nz[:, a] & (lo > tn), lo, tn)
            tf = np.where(nz[:, a], np.fmin(tf, hi), tf)
            alive &= nz[:, a] | ((o[:, a] >= 0) & (o[:, a] < dims[a]))
        t = np.where(tn > 0, tn, T(0)).astype(dtype)
        alive &= tf >= t
        p = o + d * t[:, None]
        idx = np.fmin(np.fmax(np.floor(p), T(0)), dims - T(1))
        idx = np.where(np.isfinite(idx), idx, 0).astype(np.int64)
        step = np.sign(d).astype(np.int64)
        m = np.where(step != 0, ((idx + (step > 0)).astype(dtype) - o) * inv, inf).astype(dtype)
        hit = np.full(n, -1, dtype=np.int64)
        for _ in range(X + Y + Z + 3):
            act = np.nonzero(alive)[0]
            if act.size == 0:
                break
            i = idx[act]
            vox = (i[:, 0] * Y + i[:, 1]) * Z + i[:, 2]
            visible[vox] = 1
            if trace:
                visits.append((act, vox))
            lab = flat[vox]
            occ = (lab > 0) & (lab < 255)
            hit[act[occ]] = vox[occ]
            alive[act[occ]] = False
            act = act[~occ]
            mm = m[act]
            ax = np.where((mm[:, 0] <= mm[:, 1]) & (mm[:, 0] <= mm[:, 2]), 0, np.where(mm[:, 1] <= mm[:, 2], 1, 2))
            mv = mm[np.arange(act.size), ax]
            go = mv < inf
            alive[act[~go]] = False
            act, ax = act[go], ax[go]
            idx[act, ax] += step[act, ax]
            ok = (idx[act, ax] >= 0) & (idx[act, ax] < idims[ax])
            alive[act[~ok]] = False
            act, ax = act[ok], ax[ok]
            m[act, ax] = ((idx[act, ax] + (step[act, ax] > 0)).astype(dtype) - o[act, ax]) * inv[act, ax]
        assert not alive.any(), "the step bound was reached"
    out = (visible.reshape(X, Y, Z), hit.reshape(shape).astype(np.int32))
    if trace:
        out += ((np.concatenate([v[0] for v in visits]), np.concatenate([v[1] for v in visits])) if visits
                else (np.zeros(0, np.int64), np.zeros(0, np.int64)),)
    return out


# tests/test_render.py's scenes, with the small scene's oblique image at 29 x 47: the image sizes are chosen so that the
# restatement alone passes the check below.  (At 28 x 45 six of its 1260 rays, all misses in both precisions, pass a voxel
# edge within float32 rounding of a tie and go round the other corner voxel: equal hits, two voxels marked differently.)
SCENES = {"24x20x12": ((24, 20, 12), (19, 61), (29, 47)), "64x64x16": ((64, 64, 16), (37, 122), (91, 122))}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_hits_are_cast_ref_hits_and_float32_moves_only_the_rays_float32_moves(name):
    """carve_ref's hits are cast_ref's, and its float32 run against its float64 run: the two marked volumes disagree only
    on voxels of rays whose hits differ (whose share tests/test_render.py caps at 1e-3)."""
    dims, cam_hw, obl_hw = SCENES[name]
    vol = make_scene(dims, seed=3)
    for vname, (view, (H, W)) in scene_views(dims, cam_hw, 2, obl_hw).items():
        runs = {}
        for dtype in (np.float32, np.float64):
            o, d = rays(view, H, W, dtype)
            visible, hit, (ray, vox) = carve_ref(vol, o, d, dtype, trace=True)
            assert np.array_equal(hit, cast_ref(vol, o, d, dtype)[0]), (name, vname, dtype)
            assert visible.dtype == np.uint8 and set(np.unique(visible).tolist()) <= {0, 1}
            assert visible.reshape(-1)[hit[hit >= 0]].all()                 # the first occupied voxel is marked itself
            runs[dtype] = (visible, hit.reshape(-1), ray, vox)
        (v32, h32, r32, x32), (v64, h64, r64, x64) = runs[np.float32], runs[np.float64]
        moved = h32 != h64                                                   # the rays float32 alone moves (test_render.py caps them)
        assert moved.mean() <= 1e-3, (name, vname, moved.mean())
        allowed = np.zeros(vol.size, dtype=bool)
        allowed[x32[moved[r32]]] = True
        allowed[x64[moved[r64]]] = True
        differ = (v32 != v64).reshape(-1)
        print(f"{name} {vname}: marked {v64.mean():.3f}, rays moved {int(moved.sum())}, voxels differing {int(differ.sum())}")
        assert not (differ & ~allowed).any(), (name, vname, int((differ & ~allowed).sum()))
        assert 0.02 < v64.mean() < 0.98                                      # the view does carve, and does leave something hidden


# ----------------------------------------------------------------------------------------------------- properties
def forward_camera(position_m, width, origin):
    """A pinhole of `width` pixels (KITTI's focal length scaled to it) at `position_m` looking along +x, z up -> view."""
    k, _ = kitti_calibration(width)
    E = np.eye(4)
    E[:3, :3] = [[0, -1, 0], [0, 0, -1], [1, 0, 0]]                         # sensor (x fwd, y left, z up) -> camera (x right, y down, z fwd)
    E[:3, 3] = -E[:3, :3] @ np.asarray(position_m, dtype=np.float64)
    return render.camera_view(torch.from_numpy(k), torch.from_numpy(E), origin, KITTI_VOXEL).numpy()


def pixel_of(view, points):
    """Grid points (n, 3) -> the continuous (fu, fv) = (u + 1/2, v + 1/2) they project to and their depth t, float64."""
    g = np.asarray(view, dtype=np.float64)
    assert not g[3:9].any()                                                  # a pinhole: one origin
    sol = np.linalg.solve(np.stack([g[9:12], g[12:15], g[15:18]], 1), (points - g[0:3]).T).T      # t, t fu, t fv
    with np.errstate(all="ignore"):                                          # depth 0: the camera's own plane
        return sol[:, 1] / sol[:, 0], sol[:, 2] / sol[:, 0], sol[:, 0]


def faces_inside(view, H, W, corners):
    """corners (n, 4, 3): the faces whose four corners all project inside the image, in front of the camera."""
    fu, fv, t = pixel_of(view, corners.reshape(-1, 3))
    ok = (t > 0) & (fu >= 0) & (fu <= W) & (fv >= 0) & (fv <= H)
    return ok.reshape(-1, 4).all(1)


def test_nothing_behind_a_full_wall_and_its_first_layer_inside_the_frustum():
    dims, (H, W), wall = (32, 24, 12), (48, 160), 20
    vol = np.zeros(dims, dtype=np.uint8)
    vol[wall:wall + 2] = 13                                                  # two layers thick, the whole cross-section
    origin = (0.0, -2.4, -1.0)
    view = forward_camera((0.3, 0.1, 0.2), W, origin)                       # inside the grid, in front of the wall
    visible, hit = carve_ref(vol, *rays(view, H, W, np.float32), np.float32)
    assert (hit >= 0).any() and not visible[wall + 1:].any()                # rays end on the wall or leave by a side: nothing behind is seen
    j, k = np.meshgrid(np.arange(dims[1]), np.arange(dims[2]), indexing="ij")
    corners = np.stack([np.stack([np.full(j.shape, float(wall)), j + a, k + b], -1) for a in (0, 1) for b in (0, 1)], 2)
    inside = faces_inside(view, H, W, corners.reshape(-1, 4, 3)).reshape(j.shape)
    assert 20 < inside.sum() < j.size                                        # the frustum cuts the wall
    assert visible[wall][inside].all()
    assert visible[:wall].any() and not visible[:wall].all()                # free space in front: seen inside the frustum only


def centre_ray_visibility(vol, view, voxels):
    """The voxel-centric rule this module does NOT use: a voxel is visible iff the ray from the camera to its centre
    meets no occupied voxel before it."""
    o = np.broadcast_to(np.asarray(view[0:3], dtype=np.float64), (len(voxels), 3))
    d = (voxels + 0.5) - o
    hit = cast_ref(vol, o, d, np.float64)[0]
    lin = (voxels[:, 0] * vol.shape[1] + voxels[:, 1]) * vol.shape[2] + voxels[:, 2]
    return hit == lin


def test_every_ground_voxel_in_the_frustum_is_seen_and_the_voxel_centre_rule_hides_them():
    """A ground plane from 1.7 m.  In a 160 x 320 image (f = 185 pixels, the ground from 2.9 m on) a voxel's top face
    covers 0.2 f 1.7 / d^2 >= 1.5 pixel rows out to the grid's end at d = 6.4 m, so every face inside the image holds a
    pixel centre.  (The real camera, f = 707, reaches one row per voxel at 15.5 m: camera_rays' scale is for beyond.)"""
    dims, (H, W) = (32, 24, 12), (160, 320)
    vol = np.zeros(dims, dtype=np.uint8)
    vol[:, :, 0] = 9                                                         # one layer of road, top face at z = 1 voxel
    origin = (0.0, -2.4, 0.0)
    view = forward_camera((0.0, 0.0, KITTI_VOXEL + 1.7), W, origin)         # 1.7 m above the road
    visible, hit = carve_ref(vol, *rays(view, H, W, np.float32), np.float32)
    i, j = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), indexing="ij")
    corners = np.stack([np.stack([i + a, j + b, np.ones(i.shape)], -1) for a in (0, 1) for b in (0, 1)], 2)
    inside = faces_inside(view, H, W, corners.reshape(-1, 4, 3)).reshape(i.shape)
    assert inside[-1].any() and inside.sum() > 150                           # out to the grid's end
    assert visible[:, :, 0][inside].all()
    ground = np.stack([i[inside], j[inside], np.zeros(int(inside.sum()), dtype=np.int64)], -1)
    by_centre = centre_ray_visibility(vol, view, ground)
    assert by_centre.mean() < 0.1, by_centre.mean()                          # the centre sits 0.1 m under the face: its ray enters earlier
    assert not visible[:, :, 0].all()                                        # and the road outside the frustum stays unseen


def test_edge_cases():
    vol = np.zeros((4, 3, 2), dtype=np.uint8)
    vol[2, 1, 1] = 5
    lin = lambda x, y, z: (x * 3 + y) * 2 + z

    def f(o, d, labels=vol):
        visible, hit = carve_ref(labels, np.array([o], dtype=np.float32), np.array([d], dtype=np.float32), np.float32)
        return sorted(np.nonzero(visible.reshape(-1))[0].tolist()), int(hit[0])

    # the camera outside the grid, an axis-parallel ray: enters at x = 0, marks up to and including the occupied voxel
    assert f((-2.0, 1.5, 1.5), (1, 0, 0)) == ([lin(0, 1, 1), lin(1, 1, 1), lin(2, 1, 1)], lin(2, 1, 1))
    assert f((-2.0, 1.5, 0.5), (1, 0, 0)) == ([lin(x, 1, 0) for x in range(4)], -1)       # leaves the grid: all it crossed
    assert f((-2.0, 3.5, 0.5), (1, 0, 0)) == ([], -1)                                     # parallel and outside: nothing
    assert f((1.5, 1.5, 5.0), (0, 0, -1)) == ([lin(1, 1, 0), lin(1, 1, 1)], -1)           # from above, parallel to two axes
    assert f((2.5, 1.5, 1.5), (0, 0, 0)) == ([lin(2, 1, 1)], lin(2, 1, 1))                # inside an occupied voxel
    assert f((0.5, 1.5, 1.5), (0, 0, 0)) == ([lin(0, 1, 1)], -1)                          # nothing to cross: its own voxel
    assert f((np.nan, 1.5, 1.5), (1, 0, 0)) == ([], -1) and f((0.5, 1.5, 1.5), (np.inf, 0, 0)) == ([], -1)
    # 255 is seen through, and marked
    unknown = vol.copy()
    unknown[1, 1, 1] = 255
    assert f((-2.0, 1.5, 1.5), (1, 0, 0), unknown) == ([lin(0, 1, 1), lin(1, 1, 1), lin(2, 1, 1)], lin(2, 1, 1))
    # 2-byte labels: 300 and 261 (low byte 5) are past 254, hence transparent
    wide = vol.astype(np.uint16)
    wide[0, 1, 1], wide[1, 1, 1] = 300, 261
    assert f((-2.0, 1.5, 1.5), (1, 0, 0), wide) == ([lin(0, 1, 1), lin(1, 1, 1), lin(2, 1, 1)], lin(2, 1, 1))
    # a tie between x and y: x is crossed first, so (1, 0) is visited and (0, 1) is not
    assert f((-1.0, -1.0, 0.5), (1, 1, 0))[0] == [lin(0, 0, 0), lin(1, 0, 0), lin(1, 1, 0), lin(2, 1, 0), lin(2, 2, 0), lin(3, 2, 0)]


def test_camera_rays_scale_keeps_the_frustum():
    dims = (24, 20, 12)
    k, E = kitti_calibration(61)
    args = (torch.from_numpy(k), torch.from_numpy(E), kitti_origin(dims), KITTI_VOXEL)
    view, size = vis.camera_rays(*args, (19, 61))
    assert size == (19, 61) and torch.equal(view, render.camera_view(*args)) and view.dtype == torch.float32
    fine, fine_size = vis.camera_rays(*args, (19, 61), scale=2.0)
    assert fine_size == (38, 122)
    o1, d1 = rays(view.numpy(), 19, 61, np.float64)
    o2, d2 = rays(fine.numpy(), 38, 122, np.float64)
    # ray (u, v) of the camera runs midway between rays (2u, 2v) and (2u + 1, 2v + 1) of the fine view: the same frustum
    # (directions have camera depth 1 and are affine in the pixel, so the midpoint is exact up to the views' float32)
    assert np.abs((d2[0::2, 0::2] + d2[1::2, 1::2]) / 2 - d1).max() < 1e-5 and np.abs(o1 - o2[0::2, 0::2]).max() == 0
    assert vis.camera_rays(*args, (19, 61), scale=0.5)[1] == (10, 31)
    with pytest.raises(ValueError):
        vis.camera_rays(*args, (19, 61), scale=0.0)
    with pytest.raises(ValueError):
        vis.camera_rays(*args, (0, 61))


# ----------------------------------------------------------------------------------------------------- vote_weights
def test_vote_weights():
    visible = torch.tensor([[[1, 0], [1, 0]], [[0, 1], [0, 0]]], dtype=torch.uint8)
    mask = torch.tensor([1, 1, 0, 0, 1, 1, 1, 0], dtype=torch.bool)
    w = vis.vote_weights(visible, mask, 4, 1)
    assert w.dtype == torch.uint8 and tuple(w.shape) == (2, 2, 2) and w.is_contiguous()
    assert w.reshape(-1).tolist() == [4, 1, 0, 0, 1, 4, 1, 0]
    assert vis.vote_weights(visible, None, 255, 0).reshape(-1).tolist() == [255, 0, 255, 0, 0, 255, 0, 0]
    assert vis.vote_weights(visible.bool(), mask.to(torch.uint8) * 7, 1, 1).reshape(-1).tolist() == [1, 1, 0, 0, 1, 1, 1, 0]
    for bad in ((0, 1), (256, 1), (4, -1), (4, 256), (1.5, 1), (4, 0.5)):
        with pytest.raises(ValueError, match="w_visible"):
            vis.vote_weights(visible, mask, *bad)
    with pytest.raises(ValueError, match="mask"):
        vis.vote_weights(visible, mask[:5], 4, 1)


# ----------------------------------------------------------------------------------------------------- weighted restatements
def _flat_index(idx, dims):
    X, Y, Z = dims
    return (np.clip(idx[..., 0], 0, X - 1) * Y + np.clip(idx[..., 1], 0, Y - 1)) * Z + np.clip(idx[..., 2], 0, Z - 1)


def weighted_votes(P, keys, labels, weight, origin, dims, C, v=V):
    """What integrate leaves in the bricks `keys` for one frame -> (brick, voxel, class, weight) of every vote cast."""
    Aq, cq, _ = ref_coefficients(P, keys, origin, v)
    idx = fixed_index(Aq, cq)
    lab = voting_labels(idx, labels, weight, dims, C)                       # weight as the mask: 0 does not vote
    n, vox = np.nonzero(lab >= 0)
    w = np.asarray(weight).reshape(-1).astype(np.int64)[_flat_index(idx, dims)[n, vox]]
    return n, vox, lab[n, vox], w


class WeightedMapRef(MapRef):
    """MapRef whose frames may vote with a uint8 weight per voxel; the counters stay unbounded int64 (saturating sums of
    non-negative weights commute: min(sum, 65535) is what any order of saturating adds leaves)."""

    def integrate(self, labels, P, mask=None, weight=None):
        if weight is None:
            return super().integrate(labels, P, mask)
        assert mask is None
        self._bricks = None
        keys = generous_bricks(P, self.origin, self.dims, self.v)
        n, vox, cls, w = weighted_votes(P, keys, labels, weight, self.origin, self.dims, self.C, self.v)
        world = B * keys[n] + LOCAL[vox]
        for key, c, amount in zip(map(tuple, world.tolist()), cls.tolist(), w.tolist()):
            self.votes.setdefault(key, np.zeros(self.C, dtype=np.int64))[c] += amount
        return self


def sample_ref_weighted(map_ref, P, own=None, own_weight=None, min_obs=1, exclude_self=False, keep_own=False):
    """occd_map_sample_weighted restated: the saturated map with this frame's weights retracted (from a counter that is
    neither 65535 nor below the weight), then the unweighted decision."""
    if not exclude_self:
        return sample_ref(map_ref, P, own, None, min_obs, False, keep_own)
    less = MapRef(map_ref.C, map_ref.origin, map_ref.dims, map_ref.v)
    if map_ref.votes:                                                        # one saturated copy; the rows are views into it
        less.votes = dict(zip(map_ref.votes, np.minimum(np.stack(list(map_ref.votes.values())), 65535)))
    keys = generous_bricks(P, map_ref.origin, map_ref.dims, map_ref.v)
    n, vox, cls, amount = weighted_votes(P, keys, own, own_weight, map_ref.origin, map_ref.dims, map_ref.C, map_ref.v)
    world = B * keys[n] + LOCAL[vox]
    for key, c, a in zip(map(tuple, world.tolist()), cls.tolist(), amount.tolist()):
        vec = less.votes.get(key)
        if vec is not None and vec[c] != 65535 and vec[c] >= a:
            vec[c] -= a
    return sample_ref(less, P, own, None, min_obs, False, keep_own)


def weighted_frames(dims, C, seed, n, label_bytes=1):
    """n frames of labels (frames_for's) with random weights in 0..255, a third of them 0."""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for lab, _ in frames_for(dims, C, seed, n, label_bytes):
        w = rng.integers(0, 256, dims).astype(np.uint8)
        w[rng.random(dims) < 0.33] = 0
        out.append((lab, w))
    return out


def test_weighted_restatement_reduces_to_the_unweighted_one():
    dims, C = (16, 12, 8), 5
    origin = GRIDS[dims]
    a, b = WeightedMapRef(C, origin, dims), MapRef(C, origin, dims)
    frames, poses = frames_for(dims, C, 31, 4, masked=True), sequence(dims)
    for (lab, mask), P in zip(frames, poses):
        a.integrate(lab, P, weight=mask.astype(np.uint8))
        b.integrate(lab, P, mask)
    assert set(a.votes) == set(b.votes) and all(np.array_equal(a.votes[w], b.votes[w]) for w in b.votes)
    for flags in ((False, False), (True, False), (True, True)):
        got = sample_ref_weighted(a, poses[2], frames[2][0], frames[2][1].astype(np.uint8), 1, *flags)
        want = sample_ref(b, poses[2], frames[2][0], frames[2][1], 1, *flags)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # and a weight counts as that many votes of one frame
    heavy, plain = WeightedMapRef(C, origin, dims), MapRef(C, origin, dims)
    heavy.integrate(frames[0][0], poses[0], weight=np.full(dims, 3, dtype=np.uint8))
    for _ in range(3):
        plain.integrate(frames[0][0], poses[0])
    assert all(np.array_equal(heavy.votes[w], plain.votes[w]) for w in plain.votes) and len(heavy.votes) == len(plain.votes)


# ----------------------------------------------------------------------------------------------------- the kernel stand-ins
class WeightedStandIn:
    """hip.frame_visibility, hip.map_integrate_weighted and hip.map_sample_weighted on CPU tensors, from what the host
    side hands over (the style of tests/test_map.py's KernelStandIn and tests/test_map_sample.py's SampleStandIn)."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "frame_visibility", self.frame_visibility)
        monkeypatch.setattr(hip, "map_integrate_weighted", self.integrate)
        monkeypatch.setattr(hip, "map_sample_weighted", self.sample)
        return self

    def frame_visibility(self, labels, view, size, return_hit=False):
        assert labels.dim() == 3 and view.dtype == torch.float32 and tuple(view.shape) == (18,) and labels.is_contiguous()
        lab = labels.numpy()
        lab = lab.view(np.uint16) if lab.dtype == np.int16 else lab
        self.calls.append({"kind": "visibility", "size": tuple(size), "view": view.numpy().copy()})
        visible, hit = carve_ref(lab, *rays(view.numpy(), int(size[0]), int(size[1]), np.float32), np.float32)
        return (torch.from_numpy(visible), torch.from_numpy(hit)) if return_hit else torch.from_numpy(visible)

    @staticmethod
    def _values(t):
        a = t.numpy().reshape(-1)
        return (a.view(np.uint16) if a.dtype == np.int16 else a).astype(np.int64)

    def _votes(self, table, labels, weight, dims, C):
        for row in table:
            idx = fixed_index(row[4:13].reshape(3, 3), row[None, 13:16])
            lab = voting_labels(idx, labels, weight, dims, C)[0]
            vox = np.nonzero(lab >= 0)[0]
            yield row[0], vox, lab[vox], weight[_flat_index(idx, dims)[0, vox]]

    def integrate(self, votes, table, labels, dims, n_classes, weight, table_host=None):
        v, t = KernelStandIn._u16(votes), table.numpy().astype(np.int64)
        assert t.shape[1] == 16 and len(set(t[:, 0].tolist())) == len(t) and t[:, 0].min() >= 0 and t[:, 0].max() < len(v)
        assert table_host is not None and torch.equal(table_host, table)
        assert weight.dtype == torch.uint8 and weight.numel() == labels.numel() and weight.is_contiguous()
        self.calls.append({"kind": "integrate", "n": len(t), "weight": weight.clone()})
        for slot, vox, cls, w in self._votes(t, self._values(labels), self._values(weight), dims, n_classes):
            v[slot, vox, cls] = np.minimum(v[slot, vox, cls].astype(np.int64) + w, 65535).astype(np.uint16)
        return votes

    def sample(self, votes, table, cells, own, dims, n_classes, Bq, dq, grid, own_weight=None, min_obs=1, exclude_self=False,
               keep_own=False, table_host=None):
        assert own_weight is None or (own_weight.dtype == torch.uint8 and own_weight.numel() == dims[0] * dims[1] * dims[2])
        assert own_weight is not None or not exclude_self
        self.calls.append({"kind": "sample", "exclude_self": exclude_self, "keep_own": keep_own, "min_obs": min_obs,
                           "weight": None if own_weight is None else own_weight.clone()})
        pool = votes.clone()
        if exclude_self:                                                     # retract per world voxel, then decide as ever
            v, t = KernelStandIn._u16(pool), table.numpy().astype(np.int64)
            for slot, vox, cls, w in self._votes(t, self._values(own), self._values(own_weight), dims, n_classes):
                cur = v[slot, vox, cls].astype(np.int64)
                v[slot, vox, cls] = np.where((cur != 65535) & (cur >= w), cur - w, cur).astype(np.uint16)
        return SampleStandIn().sample(pool, table, cells, own, dims, n_classes, Bq, dq, grid, None, min_obs, False, keep_own,
                                      table_host)


def _tensor(a):
    return torch.from_numpy(a if a.dtype != np.uint16 else a.view(np.int16))


@pytest.mark.parametrize("dims,C,label_bytes", [((16, 12, 8), 5, 1), ((40, 24, 20), 7, 2)])
def test_semantic_map_weighted_on_the_stand_ins_equals_the_restatement(monkeypatch, dims, C, label_bytes):
    k = KernelStandIn().install(monkeypatch)
    w = WeightedStandIn().install(monkeypatch)
    origin = GRIDS[dims]
    m, ref = sm.SemanticMap(C, V, origin, dims, chunk_bricks=8), WeightedMapRef(C, origin, dims)
    frames, poses = weighted_frames(dims, C, 51, 4, label_bytes), sequence(dims)
    for (lab, weight), P in zip(frames[:3], poses):
        assert m.integrate(_tensor(lab), P, weight=torch.from_numpy(weight)) is m
        ref.integrate(lab, P, weight=weight)
    plain, plain_mask = frames_for(dims, C, 52, 1, label_bytes, masked=True)[0]       # both kinds of frame share one map
    m.integrate(_tensor(plain), poses[3], mask=torch.from_numpy(plain_mask))
    ref.integrate(plain, poses[3], plain_mask)
    assert_map_equals_ref(m, ref)
    assert [c["kind"] for c in w.calls] == ["integrate"] * 3 and len(k.calls) == 1
    for i, P in enumerate(poses[:3]):
        own, weight = frames[i]
        for flags in ((False, False), (True, False), (False, True), (True, True)):
            got = m.sample(P, own=_tensor(own), own_weight=torch.from_numpy(weight), min_obs=1 + 40 * i, exclude_self=flags[0],
                           keep_own=flags[1])
            want = sample_ref_weighted(ref, P, own, weight, 1 + 40 * i, *flags)
            assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy().view(np.uint16), want[1]), (i, flags)
    assert (want[1] > 255).any()                                             # n_obs counts vote units, not frames


def test_refusals(monkeypatch):
    dims, C = (16, 12, 8), 5
    m = sm.SemanticMap(C, V, GRIDS[dims], dims)
    lab, weight = torch.zeros(dims, dtype=torch.uint8), torch.ones(dims, dtype=torch.uint8)
    with pytest.raises(ValueError, match="not both"):
        m.integrate(lab, pose(), mask=weight.bool(), weight=weight)
    with pytest.raises(ValueError, match="not both"):
        m.sample(pose(), own=lab, own_mask=weight.bool(), own_weight=weight)
    for bad in (weight.to(torch.int16), weight[:3], weight.float()):
        with pytest.raises(ValueError, match="uint8 weights"):
            m.integrate(lab, pose(), weight=bad)
        with pytest.raises(ValueError, match="uint8 weights"):
            m.sample(pose(), own=lab, own_weight=bad)
    assert m.n_bricks == 0 and m.votes is None                              # a refusal admits no brick
    pool, table = torch.zeros((1, B ** 3, 8), dtype=torch.int16), torch.zeros((1, 16), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="weight"):
        hip.map_integrate_weighted(pool, table, lab, dims, C, None)
    with pytest.raises(RuntimeError, match="uint8 weights"):
        hip.map_integrate_weighted(pool, table, lab, dims, C, weight.bool())
    with pytest.raises(RuntimeError, match="own_weight"):
        hip.map_sample_weighted(pool, table, torch.zeros((1, 1, 1), dtype=torch.int32), lab, dims, C, np.eye(3, dtype=np.int32),
                                np.zeros(3, dtype=np.int32), (1, 1, 1), exclude_self=True)
    with pytest.raises(RuntimeError, match="GPU"):                           # no CPU path behind the binding
        hip.frame_visibility(lab, torch.zeros(18), (4, 4))
    with pytest.raises(RuntimeError, match="18"):
        hip.frame_visibility(lab, torch.zeros(17), (4, 4))
    with pytest.raises(RuntimeError, match="X, Y, Z"):
        hip.frame_visibility(lab[None], torch.zeros(18), (4, 4))
    with pytest.raises(ValueError, match="X, Y, Z"):
        vis.visible_voxels(lab[None], torch.zeros(18), (4, 4))
    with pytest.raises(ValueError, match="18"):
        vis.visible_voxels(lab, torch.zeros(12), (4, 4))


# ----------------------------------------------------------------------------------------------------- the model hook
CALIB = ("P2: 40 0 12 4 0 40 6 0.2 0 0 1 0.001\n"
         "Tr: 0 -1 0 0.5 0 0 -1 0.25 1 0 0 -0.125\n")


def _write_sequence(d, poses):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "poses.txt"), "w") as f:
        f.write(poses)
    with open(os.path.join(d, "calib.txt"), "w") as f:
        f.write(CALIB)
    return str(d)


HOOK_HW = (12, 24)
HOOK_K = np.array([[40.0, 0, 12], [0, 40.0, 6], [0, 0, 1]])
HOOK_E = np.array([[0.0, -1, 0, 0.0], [0, 0, -1, 0.1], [1, 0, 0, 1.0], [0, 0, 0, 1]])       # the camera 1 m behind the grid's first plane


def _camera_steps():
    steps = _hook_steps()
    for batch, logits, _ in steps:
        n = len(batch["frame_id"])
        batch["cam_k"] = [torch.from_numpy(HOOK_K).float() for _ in range(n)]
        batch["T_velo_2_cam"] = [torch.from_numpy(HOOK_E).float() for _ in range(n)]
        batch["img"] = torch.zeros((n, 2, 3) + HOOK_HW)
    return steps


def _install(monkeypatch):
    k, s, w = KernelStandIn().install(monkeypatch), SampleStandIn().install(monkeypatch), WeightedStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    return k, s, w


def test_model_hook_votes_with_visibility_weights(monkeypatch, tmp_path):
    from occdepth_amd import fuse
    from occdepth_amd.models.OccDepth import OccDepth
    k, s, w = _install(monkeypatch)
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    steps = _camera_steps()

    # off (the default): the weighted kernels and the visibility pass are never reached
    off = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "off"), str(root), frames=True)
    assert off.semantic_map["visibility"] is None
    _epoch(off, "val", steps)
    assert not w.calls and len(k.calls) == 8 and len(s.calls) == 4

    k.calls.clear()
    s.calls.clear()
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "on"), str(root), frames=True,
                                        exclude_self=True, visibility=(6, 1))
    assert stub.semantic_map["visibility"] == (6, 1)
    for batch, logits, target in steps[:1]:                                  # mid-epoch: the kept frames hold the weights
        OccDepth._map_step(stub, "val", batch, logits, target)
    kept = stub.semantic_map["kept"][("val", "08")]
    assert len(kept) == 2 and kept[0][2].dtype == torch.uint8 and tuple(kept[0][2].shape) == HOOK_DIMS
    assert set(kept[0][2].unique().tolist()) <= {0, 1, 6} and (kept[0][2] == 6).any() and (kept[0][2] == 1).any()
    stub.semantic_map["maps"].clear()
    stub.semantic_map["kept"].clear()
    w.calls.clear()
    k.calls.clear()
    _epoch(stub, "val", steps)
    kinds = [c["kind"] for c in w.calls]
    assert kinds.count("visibility") == 4 and kinds.count("integrate") == 4 and kinds.count("sample") == 4
    assert len(k.calls) == 4 and all(c["mask"] and c["dtype"] == torch.uint8 for c in k.calls)     # the ground truth: unchanged
    assert not s.calls and all(c["exclude_self"] and c["keep_own"] for c in w.calls if c["kind"] == "sample")
    assert all(c["size"] == HOOK_HW for c in w.calls if c["kind"] == "visibility")
    assert set(stub.logged_keys) == set(off.logged_keys)
    assert np.array_equal(stub.logged_keys["val/mIoU"], off.logged_keys["val/mIoU"])

    # the weights are those of the restated walk through the predicted labels; the mapped score is the restatement's
    vs = 0.2
    view = render.camera_view(torch.from_numpy(HOOK_K), torch.from_numpy(HOOK_E), HOOK_ORIGIN, vs).numpy()
    want = np.zeros((HOOK_C, HOOK_C), dtype=np.int64)
    n_weights = 0
    for seq in ("03", "08"):
        poses = fuse.read_kitti_poses(str(root / seq))
        ref = WeightedMapRef(HOOK_C, HOOK_ORIGIN, HOOK_DIMS, vs)
        mine = []
        for batch, logits, target in steps:
            for i, q in enumerate(batch["sequence"]):
                if q == seq:
                    pred = logits[i].argmax(0).numpy().astype(np.uint8)
                    visible, _ = carve_ref(pred, *rays(view, *HOOK_HW, np.float32), np.float32)
                    weight = np.where(visible != 0, 6, 1).astype(np.uint8) * batch["fov_mask_1"][i].numpy().reshape(HOOK_DIMS)
                    assert any(np.array_equal(c["weight"].numpy(), weight) for c in w.calls if c["kind"] == "integrate")
                    n_weights += 1
                    mine.append((pred, target[i].numpy(), weight, poses[int(batch["frame_id"][i])]))
        for pred, _, weight, P in mine:
            ref.integrate(pred, P, weight=weight)
        for pred, target, weight, P in mine:
            mapped, _ = sample_ref_weighted(ref, P, pred, weight, 1, True, True)
            keep = target != 255
            np.add.at(want, (target[keep].astype(np.int64), mapped[keep].astype(np.int64)), 1)
    assert n_weights == 4 and want.sum() > 0 and np.array_equal(stub.hists[-2].numpy(), want)

    # refusals
    for bad in ((0, 1), (4,), (4, 1, 2), (300, 1), (4, -1)):
        with pytest.raises(ValueError):
            OccDepth.enable_semantic_map(_hook_stub(), str(tmp_path), str(root), visibility=bad)
    blind = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "x"), str(root), visibility=(4, 1))
    with pytest.raises(KeyError, match="cam_k"):
        OccDepth._map_step(blind, "val", *_hook_steps()[0])                  # a batch without its camera


def test_map_visibility_is_switched_by_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def state():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg).semantic_map

    for var in ("OCCDEPTH_MAP_VISIBILITY", "OCCDEPTH_MAP_FRAMES", "OCCDEPTH_MAP_FRAMES_SELF", "OCCDEPTH_MAP_SUBMISSION",
                "OCCDEPTH_MAP_MIN_OBS", "OCCDEPTH_MAP_VIEWS", "OCCDEPTH_FUSE", "OCCDEPTH_FUSE_POSES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OCCDEPTH_MAP_DIR", str(tmp_path / "maps"))
    monkeypatch.setenv("OCCDEPTH_MAP_POSES", str(tmp_path / "seq"))
    assert state()["visibility"] is None
    monkeypatch.setenv("OCCDEPTH_MAP_VISIBILITY", "8,1")
    assert state()["visibility"] == (8, 1)
    monkeypatch.setenv("OCCDEPTH_MAP_VISIBILITY", "8")
    with pytest.raises(ValueError, match="OCCDEPTH_MAP_VISIBILITY"):
        state()
    monkeypatch.setenv("OCCDEPTH_MAP_VISIBILITY", "0,1")
    with pytest.raises(ValueError, match="w_visible"):
        state()


# ----------------------------------------------------------------------------------------------------- the offline tool
def test_map_sequence_tool_takes_visibility_weights(monkeypatch, tmp_path, capsys):
    from occdepth_amd import fuse, output
    tool = _tool()
    k, s, w = _install(monkeypatch)
    dims, C = (16, 12, 8), 20
    origin = (0.0, -1.2, -0.8)
    seq = _write_sequence(tmp_path / "08", "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 0.4\n1 0 0 0.2 0 1 0 0 0 0 1 1.0\n")
    frames = frames_for(dims, C, 21, 3, masked=True)
    pkl = tmp_path / "pkl"
    os.makedirs(pkl)
    for n, (lab, mask) in enumerate(frames):
        with open(pkl / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": lab.astype(np.uint16), "target": np.roll(lab, 1, axis=0).astype(np.uint16),
                         "fov_mask_1": mask.reshape(-1)}, f)
    base = ["--poses", seq, "--pred", str(pkl), "--gt", str(pkl), "--out", str(tmp_path / "m" / "08"), "--dims", "16", "12", "8",
            "--origin"] + [str(o) for o in origin] + ["--fov", "--camera-size", "12", "24"]
    assert tool.parser().parse_args(base).visibility is None
    tool.run(tool.parser().parse_args(base), device=torch.device("cpu"))
    assert not w.calls                                                       # without the switch nothing new is reached
    out_dir = tmp_path / "frames"
    maps, _ = tool.run(tool.parser().parse_args(base + ["--visibility", "5", "2", "--frames-out", str(out_dir), "--exclude-self"]),
                       device=torch.device("cpu"))
    kinds = [c["kind"] for c in w.calls]
    assert kinds == ["visibility", "integrate"] * 3 + ["visibility", "sample"] * 3 and not s.calls
    cam_k, E = tool.read_camera(seq)
    assert np.array_equal(cam_k, [[40, 0, 12], [0, 40, 6], [0, 0, 1]]) and np.allclose(E[:3, 3], [0.5 + (4 - 0.012) / 40, 0.25 + (0.2 - 0.006) / 40, -0.124])
    view = render.camera_view(torch.from_numpy(cam_k), torch.from_numpy(E), origin, V).numpy()
    poses = fuse.read_kitti_poses(seq)
    ref, gt_ref = WeightedMapRef(C, origin, dims), MapRef(C, origin, dims)
    weights = []
    for n, (lab, mask) in enumerate(frames):
        visible, _ = carve_ref(np.minimum(lab, 255), *rays(view, 12, 24, np.float32), np.float32)
        weights.append(np.where(visible != 0, 5, 2).astype(np.uint8) * mask)
        ref.integrate(lab, poses[n], weight=weights[-1])
        gt_ref.integrate(np.roll(lab, 1, axis=0), poses[n], mask)
    assert any((wt == 5).any() and (wt == 2).any() and (wt == 0).any() for wt in weights)
    assert_map_equals_ref(maps["pred"], ref)
    assert_map_equals_ref(maps["gt"], gt_ref)                                # the ground-truth map votes as it always did
    ids = np.array(output.KITTI_LEARNING_MAP_INV + (0,) * 236, dtype=np.uint16)
    for n, (lab, mask) in enumerate(frames):
        mapped, _ = sample_ref_weighted(ref, poses[n], np.minimum(lab, 255), weights[n], 1, True, False)
        got = np.fromfile(str(out_dir / "sequences" / "08" / "predictions" / ("%06d.label" % n)), dtype=np.uint16)
        assert np.array_equal(got, ids[mapped.reshape(-1)])


# ----------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_validate_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected
    host16 = np.zeros((2, 16), dtype=np.int32)

    def visibility():
        a = hip.VisibilityArgs()
        a.labels = a.view = a.visible = a.hit = ptr
        a.H, a.W, a.X, a.Y, a.Z, a.label_bytes = 48, 160, 40, 24, 20, 1
        return a

    fn = hip_lib.occd_frame_visibility
    assert fn(None, None) == -1
    for field, value in (("labels", None), ("view", None), ("visible", None), ("H", 0), ("W", -1), ("X", 0), ("Y", -2), ("Z", 0),
                         ("label_bytes", 0), ("label_bytes", 3), ("label_bytes", 4)):
        a = visibility()
        setattr(a, field, value)
        assert fn(ctypes.byref(a), None) == -1, (field, value)
    a = visibility()
    a.X, a.Y, a.Z = 1 << 10, 1 << 10, (1 << 8) + 1                          # just past 2^28 voxels
    assert fn(ctypes.byref(a), None) == -1

    def frame():
        a = hip.MapWeightedArgs()
        a.votes = a.table = a.labels = a.weight = ptr
        a.n_bricks, a.capacity, a.X, a.Y, a.Z, a.C, a.pitch, a.label_bytes = 2, 4, 40, 24, 20, 20, 20, 1
        return a

    integrate = hip_lib.occd_map_integrate_weighted
    assert integrate(None, None) == -1
    for field, value in (("votes", None), ("table", None), ("labels", None), ("weight", None), ("C", 0), ("C", 33), ("X", 0),
                         ("Y", -1), ("Z", 0), ("n_bricks", 0), ("capacity", 0), ("label_bytes", 0), ("label_bytes", 3),
                         ("pitch", 19), ("pitch", 16), ("pitch", 22), ("votes", ptr + 2)):
        a = frame()
        setattr(a, field, value)
        assert integrate(ctypes.byref(a), None) == -1, (field, value)
    a = frame()
    a.X = a.Y = a.Z = 1 << 10
    assert integrate(ctypes.byref(a), None) == -1
    for slot in (4, -1):
        a = frame()
        host16[1, 0] = slot
        a.table_host = host16.ctypes.data
        assert integrate(ctypes.byref(a), None) == -1, slot
    host16[1, 0] = 0

    def sample():
        a = hip.MapSampleWeightedArgs()
        a.votes = a.table = a.cells = a.own = a.own_weight = a.labels = a.n_obs = ptr
        a.n_bricks, a.capacity, a.X, a.Y, a.Z, a.gx, a.gy, a.gz = 2, 4, 40, 24, 20, 4, 3, 3
        a.C, a.pitch, a.label_bytes, a.min_obs, a.flags = 20, 20, 1, 1, 3
        return a

    fn = hip_lib.occd_map_sample_weighted
    assert fn(None, None) == -1
    for field, value in (("votes", None), ("table", None), ("cells", None), ("labels", None), ("n_obs", None), ("own", None),
                         ("own_weight", None), ("C", 33), ("X", 0), ("gx", 0), ("n_bricks", 0), ("capacity", 0), ("label_bytes", 3),
                         ("pitch", 16), ("min_obs", -1), ("flags", 4), ("votes", ptr + 2)):
        a = sample()
        setattr(a, field, value)
        assert fn(ctypes.byref(a), None) == -1, (field, value)
    a = sample()
    a.own_weight, a.flags = None, 1                                          # exclude_self alone still needs the weights
    assert fn(ctypes.byref(a), None) == -1
    a = sample()
    host16[1, 0] = 4
    a.table_host = host16.ctypes.data
    assert fn(ctypes.byref(a), None) == -1
    # the weighted structs are the unweighted ones with one field renamed, and the ABI version did not move
    assert hip.ABI_VERSION == 22
    assert ctypes.sizeof(hip.MapWeightedArgs) == ctypes.sizeof(hip.MapFrameArgs) and hip.MapWeightedArgs.weight.offset == hip.MapFrameArgs.mask.offset
    assert ctypes.sizeof(hip.MapSampleWeightedArgs) == ctypes.sizeof(hip.MapSampleArgs)
    assert hip.MapSampleWeightedArgs.own_weight.offset == hip.MapSampleArgs.own_mask.offset
    assert ctypes.sizeof(hip.VisibilityArgs) == 4 * 8 + 6 * 4
    for name in ("occd_frame_visibility", "occd_map_integrate_weighted", "occd_map_sample_weighted"):
        assert name in hip.EXPORTS
