"""CPU: RayIoU along sensor rays (K35, occd_ray_metric; occdepth_amd/ray_metric.py).

`ray_metric_ref` restates the kernel's counters: two independent `cast_ref` calls (tests/test_render.py, the walk of
csrc/raycast.h in float32) per origin, one through the prediction and one through the target, then plain numpy counting
with the depth test in float32.  tests/test_ray_metric_gpu.py holds the kernel to it with exact equality.  Here: the
restatement against analytic cases and edge rays, the direction fan and the trajectory origins, RayMetrics on a Python
stand-in for the kernel, the model hook, the environment switches and the offline tool on that stand-in, and the entry
point's argument checks before any launch."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd import ray_metric as rm
from test_map import HOOK_C, HOOK_DIMS, HOOK_ORIGIN, _confusion_stand_in, _hook_steps, _hook_stub
from test_render import KITTI_VOXEL, cast_ref, kitti_origin, make_scene
from test_visibility import _write_sequence

SPARE = 254                      # the occupied code target 255 is cast as in drop mode; no scene here uses it
THR_M = (1.0, 2.0, 4.0)


def grid_thresholds(thresholds_m, voxel_size=KITTI_VOXEL):
    return [np.float32(t / voxel_size) for t in thresholds_m]


# ----------------------------------------------------------------------------------------------------- the restatement
def ray_metric_ref(pred, target, origins, dirs, thresholds, n_classes, unknown="drop"):
    """pred, target (B, X, Y, Z) integer arrays; origins (B, K, 3), dirs (N, 3); thresholds in grid units -> the int64
    counters in the kernel's layout: rays, valid, unknown, pred_miss, gt[C], pred[C], tp[T][C], tp_geo[T]."""
    C, T = int(n_classes), len(thresholds)
    thr = [np.float32(t) for t in thresholds]
    origins = np.asarray(origins, dtype=np.float32)
    dirs = np.asarray(dirs, dtype=np.float32)
    B, K, N = origins.shape[0], origins.shape[1], dirs.shape[0]
    scalars = np.zeros(4, dtype=np.int64)
    gt, pr, tp, geo = np.zeros(C, np.int64), np.zeros(C, np.int64), np.zeros((T, C), np.int64), np.zeros(T, np.int64)
    for b in range(B):
        p_vol = np.asarray(pred[b]).astype(np.int64)
        g_vol = np.asarray(target[b]).astype(np.int64)
        if unknown == "drop":
            assert not (g_vol == SPARE).any()
            g_vol = np.where(g_vol == 255, SPARE, g_vol)
        for k in range(K):
            o = np.broadcast_to(origins[b, k], (N, 3))
            hit_p, _, t_p = cast_ref(p_vol, o, dirs, np.float32)
            hit_g, _, t_g = cast_ref(g_vol, o, dirs, np.float32)
            cls_p = np.where(hit_p >= 0, p_vol.reshape(-1)[np.maximum(hit_p, 0)], 0)
            cls_g = np.where(hit_g >= 0, g_vol.reshape(-1)[np.maximum(hit_g, 0)], 0)
            dropped = (cls_g == SPARE) if unknown == "drop" else np.zeros(N, dtype=bool)
            valid = ~dropped & (cls_g > 0) & (cls_g < C)
            scalars += [N, int(valid.sum()), int(dropped.sum()), int((valid & (cls_p == 0)).sum())]
            gt += np.bincount(cls_g[valid], minlength=256)[:C]
            both = valid & (cls_p > 0)
            pr += np.bincount(cls_p[both], minlength=256)[:C]
            with np.errstate(invalid="ignore"):
                diff = np.abs(t_p.astype(np.float32) - t_g.astype(np.float32))
            for i, th in enumerate(thr):
                close = both & (diff < th)
                geo[i] += int(close.sum())
                tp[i] += np.bincount(cls_g[close & (cls_p == cls_g)], minlength=256)[:C]
    return np.concatenate([scalars, gt, pr, tp.reshape(-1), geo]).astype(np.int64)


def split(counts, C, T):
    c = np.asarray(counts).reshape(-1)
    assert c.size == 4 + 2 * C + T * C + T
    return SimpleNamespace(rays=int(c[0]), valid=int(c[1]), unknown=int(c[2]), pred_miss=int(c[3]), gt=c[4:4 + C],
                           pred=c[4 + C:4 + 2 * C], tp=c[4 + 2 * C:4 + 2 * C + T * C].reshape(T, C), tp_geo=c[4 + 2 * C + T * C:])


def make_prediction(target, seed):
    """The target rolled one voxel along x, 255 -> 0, 20 % of the occupied labels redrawn."""
    rng = np.random.RandomState(seed + 9)       # a draw under which tp differs between the thresholds on every scene
    p = np.roll(target, 1, axis=0)
    p[p == 255] = 0
    redraw = (p > 0) & (rng.rand(*p.shape) < 0.2)
    p[redraw] = rng.randint(1, 20, size=int(redraw.sum()))
    return p


SCENES = {"24x20x12": ((24, 20, 12), 1), "64x64x16": ((64, 64, 16), 2), "128x128x32": ((128, 128, 32), 3)}
# what the restatement alone gives on the three scenes with 16 beams x 90 azimuths from the KITTI sensor origin, of 1440 rays
EXPECT = {"24x20x12": {"pass": (1015, 0), "drop": (915, 214)}, "64x64x16": {"pass": (1324, 0), "drop": (929, 469)},
          "128x128x32": {"pass": (1421, 0), "drop": (722, 711)}}
_scene_cache = {}


def scene(name):
    """-> target, prediction (X, Y, Z) uint8, origin (3,) float32, dirs (1440, 3) float32 and the restatement's counters
    {mode: counts} at thresholds 1 / 2 / 4 m and 20 classes: computed once, shared, never written to."""
    if name not in _scene_cache:
        dims, seed = SCENES[name]
        target = make_scene(dims, seed)
        pred = make_prediction(target, seed)
        origin = rm.sensor_origin(kitti_origin(dims), KITTI_VOXEL).numpy()
        dirs = rm.lidar_directions(beams=16, azimuth_step_deg=2.0).numpy()
        ref = {mode: ray_metric_ref(pred[None], target[None], origin[None, None], dirs, grid_thresholds(THR_M), 20, mode)
               for mode in ("pass", "drop")}
        for a in (target, pred, origin, dirs) + tuple(ref.values()):
            a.setflags(write=False)
        _scene_cache[name] = (target, pred, origin, dirs, ref)
    return _scene_cache[name]


def guard(c, mode):
    """An all-zero kernel, or one that scores nothing, cannot pass for the restatement."""
    assert c.valid >= 0.3 * c.rays and 0.1 <= c.tp[0].sum() / c.valid <= 0.9
    assert (c.unknown > 0) == (mode == "drop")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_restatement_on_the_scenes(name):
    target, pred, origin, dirs, ref = scene(name)
    assert dirs.shape == (1440, 3)
    for mode in ("pass", "drop"):
        c = split(ref[mode], 20, 3)
        print(name, mode, "valid", c.valid, "unknown", c.unknown, "pred_miss", c.pred_miss, "tp", c.tp.sum(1).tolist(),
              "tp_geo", c.tp_geo.tolist())
        assert c.rays == 1440 and (c.valid, c.unknown) == EXPECT[name][mode]
        guard(c, mode)
        assert c.pred_miss > 0 and c.gt.sum() == c.valid and c.pred.sum() == c.valid - c.pred_miss
        assert c.tp.sum(1)[0] < c.tp.sum(1)[1] < c.tp.sum(1)[2]            # the thresholds differ
        assert (c.tp_geo > c.tp.sum(1)).all() and (c.tp <= np.minimum(c.gt, c.pred)).all()
        assert c.gt[0] == 0 and c.pred[0] == 0 and not c.tp[:, 0].any()


# ----------------------------------------------------------------------------------------------------- analytic cases
def wall(dims, x, label=13):
    vol = np.zeros(dims, dtype=np.uint8)
    vol[x] = label
    return vol


def parallel_origins(dims):
    """One origin per (y, z) column, on the x = 0 face: with the single direction +x every ray is axis-parallel."""
    _, Y, Z = dims
    y, z = np.meshgrid(np.arange(Y) + 0.5, np.arange(Z) + 0.5, indexing="ij")
    return np.stack([np.zeros(y.size), y.reshape(-1), z.reshape(-1)], -1).astype(np.float32)[None]


PLUS_X = np.array([[1.0, 0.0, 0.0]], dtype=np.float32)


@pytest.mark.parametrize("shift,want", [(0, (1, 1, 1)), (4, (1, 1, 1)), (9, (0, 1, 1)), (19, (0, 0, 1)), (5, (0, 1, 1)), (20, (0, 0, 0))])
def test_a_shifted_wall_flips_tp_where_the_threshold_says(shift, want):
    """A full wall 5 voxels in, the prediction's wall `shift` voxels behind it, 0.2 m voxels: tp at 1 / 2 / 4 m iff
    shift * 0.2 < tau (strictly: 5 voxels are not within 1 m)."""
    dims, C = (32, 4, 3), 20
    target, pred = wall(dims, 5), wall(dims, 5 + shift)
    o = parallel_origins(dims)
    c = split(ray_metric_ref(pred[None], target[None], o, PLUS_X, grid_thresholds(THR_M), C), C, 3)
    n = dims[1] * dims[2]
    assert (c.rays, c.valid, c.unknown, c.pred_miss) == (n, n, 0, 0) and c.gt[13] == n and c.pred[13] == n
    assert tuple(c.tp[:, 13].tolist()) == tuple(n * w for w in want) and tuple(c.tp_geo.tolist()) == tuple(n * w for w in want)
    assert [abs(shift) * 0.2 < t for t in THR_M] == [bool(w) for w in want]
    # the other way round (the prediction in front) is the same: the test is on |t_p - t_g|
    c2 = split(ray_metric_ref(target[None], pred[None], o, PLUS_X, grid_thresholds(THR_M), C), C, 3)
    assert np.array_equal(c2.tp, c.tp)


def test_wrong_class_empty_prediction_and_identity():
    dims, C = (32, 4, 3), 20
    n = dims[1] * dims[2]
    o, thr = parallel_origins(dims), grid_thresholds(THR_M)
    target = wall(dims, 5)
    wrong = split(ray_metric_ref(wall(dims, 6, label=7)[None], target[None], o, PLUS_X, thr, C), C, 3)
    assert not wrong.tp.any() and wrong.tp_geo.tolist() == [n] * 3 and wrong.pred[7] == n and wrong.gt[13] == n
    empty = ray_metric_ref(np.zeros((1,) + dims, np.uint8), target[None], o, PLUS_X, thr, C)
    e = split(empty, C, 3)
    assert (e.valid, e.pred_miss) == (n, n) and not e.pred.any() and not e.tp.any() and not e.tp_geo.any()
    m = rm.RayMetrics(C, KITTI_VOXEL, PLUS_X).merge_(torch.from_numpy(empty))
    stats = m.get_stats()
    assert stats["RayIoU"] == 0.0 and not stats["ray_iou"].any() and not stats["ray_iou_geo"].any()
    scene_t = make_scene((24, 20, 12), 1)
    dirs = rm.lidar_directions(beams=8, azimuth_step_deg=4.0).numpy()
    org = rm.sensor_origin(kitti_origin((24, 20, 12)), KITTI_VOXEL).numpy()[None, None]
    same = ray_metric_ref(scene_t[None], scene_t[None], org, dirs, thr, C, "pass")
    stats = rm.RayMetrics(C, KITTI_VOXEL, dirs).merge_(torch.from_numpy(same)).get_stats()
    assert stats["valid"] > 100 and stats["RayIoU"] == 1.0 and (stats["ray_miou"] == 1.0).all() and (stats["ray_iou_geo"] == 1.0).all()


# ----------------------------------------------------------------------------------------------------- edge rays
def one(pred, target, o, d, C=8, mode="drop", thr=(5.0,)):
    c = split(ray_metric_ref(pred[None], target[None], np.array([[o]], np.float32), np.array([d], np.float32), thr, C, mode), C, len(thr))
    assert c.rays == 1
    return c


def test_edge_rays():
    dims = (6, 3, 2)
    target = np.zeros(dims, dtype=np.uint8)
    target[4, 1, 1] = 5
    pred = np.zeros(dims, dtype=np.uint8)
    pred[2, 1, 1] = 5
    hit = lambda c: (c.valid, c.unknown, c.pred_miss, int(c.gt[5]), int(c.pred[5]), int(c.tp[0, 5]), int(c.tp_geo[0]))
    # axis-parallel, from outside the grid: enters at x = 0, depths 4 and 6
    assert hit(one(pred, target, (-2.0, 1.5, 1.5), (1, 0, 0))) == (1, 0, 0, 1, 1, 1, 1)
    assert hit(one(pred, target, (-2.0, 1.5, 1.5), (1, 0, 0), thr=(2.0,))) == (1, 0, 0, 1, 1, 0, 0)          # |6 - 4| < 2 is false
    assert hit(one(pred, target, (-2.0, 1.5, 0.5), (1, 0, 0))) == (0, 0, 0, 0, 0, 0, 0)                        # crosses, hits nothing
    assert hit(one(pred, target, (-2.0, 3.5, 1.5), (1, 0, 0))) == (0, 0, 0, 0, 0, 0, 0)                        # parallel and outside: misses the grid
    assert hit(one(pred, target, (-2.0, 1.5, 1.5), (-1, 0, 0))) == (0, 0, 0, 0, 0, 0, 0)                       # points away
    assert hit(one(pred, target, (0.0, 1.5, 1.5), (1, 0, 0))) == (1, 0, 0, 1, 1, 1, 1)                         # on the boundary
    assert hit(one(pred, target, (4.5, 1.5, 5.0), (0, 0, -1))) == (1, 0, 1, 1, 0, 0, 0)                        # from above: the target only
    # inside an occupied voxel: depth 0 in that volume
    inside = one(pred, target, (4.5, 1.5, 1.5), (-1, 0, 0), thr=(1.5, 2.0))
    assert (inside.valid, inside.pred_miss) == (1, 0) and inside.tp[:, 5].tolist() == [0, 1]                  # t_g = 0, t_p = 1.5
    assert hit(one(pred, target, (4.5, 1.5, 1.5), (0, 0, 0))) == (1, 0, 1, 1, 0, 0, 0)                         # a zero direction: its own voxel
    # non-finite: a miss in both, still a ray
    for o, d in (((np.nan, 1.5, 1.5), (1, 0, 0)), ((-2.0, 1.5, 1.5), (np.nan, 0, 0)), ((-2.0, 1.5, 1.5), (np.inf, 0, 0)),
                 ((-np.inf, 1.5, 1.5), (1, 0, 0))):
        assert hit(one(pred, target, o, d)) == (0, 0, 0, 0, 0, 0, 0)
    # a label >= n_classes: such a target hit is not valid; such a prediction hit is no miss, no pred[c], but geometry
    out = one(pred, target, (-2.0, 1.5, 1.5), (1, 0, 0), C=5)
    assert (out.valid, out.unknown, out.pred_miss) == (0, 0, 0) and not out.gt.any() and not out.pred.any() and not out.tp_geo.any()
    big = pred.copy()
    big[2, 1, 1] = 200
    c = one(big, target, (-2.0, 1.5, 1.5), (1, 0, 0))
    assert (c.valid, c.pred_miss, int(c.pred.sum()), int(c.tp.sum()), int(c.tp_geo[0])) == (1, 0, 0, 0, 1)
    # 255 in the prediction is seen through, in both modes
    veil = pred.copy()
    veil[1, 1, 1] = 255
    for mode in ("drop", "pass"):
        assert hit(one(veil, target, (-2.0, 1.5, 1.5), (1, 0, 0), mode=mode)) == (1, 0, 0, 1, 1, 1, 1)
    # 255 in the target: dropped when it comes before the target hit, seen through in pass mode, irrelevant behind the hit
    unk = target.copy()
    unk[3, 1, 1] = 255
    assert hit(one(pred, unk, (-2.0, 1.5, 1.5), (1, 0, 0), mode="drop")) == (0, 1, 0, 0, 0, 0, 0)
    assert hit(one(pred, unk, (-2.0, 1.5, 1.5), (1, 0, 0), mode="pass")) == (1, 0, 0, 1, 1, 1, 1)
    behind = target.copy()
    behind[5, 1, 1] = 255
    assert hit(one(pred, behind, (-2.0, 1.5, 1.5), (1, 0, 0), mode="drop")) == (1, 0, 0, 1, 1, 1, 1)
    assert hit(one(pred, behind, (8.0, 1.5, 1.5), (-1, 0, 0), mode="drop")) == (0, 1, 0, 0, 0, 0, 0)
    # 2-byte labels above 255 are transparent in both volumes
    wide_t, wide_p = target.astype(np.uint16), pred.astype(np.uint16)
    wide_t[1, 1, 1], wide_p[0, 1, 1] = 300, 261
    assert hit(one(wide_p, wide_t, (-2.0, 1.5, 1.5), (1, 0, 0))) == (1, 0, 0, 1, 1, 1, 1)


# ----------------------------------------------------------------------------------------------------- helpers
def test_lidar_directions():
    d = rm.lidar_directions()
    assert d.dtype == torch.float32 and tuple(d.shape) == (64 * 900, 3)
    small = rm.lidar_directions(beams=16, azimuth_step_deg=2.0)
    plain = rm.lidar_directions(beams=16, azimuth_step_deg=2.0, tile=None)
    assert tuple(small.shape) == (1440, 3) == tuple(plain.shape)
    for v in (d, small, plain):                                             # unit length to 1 ulp of float32
        n = np.linalg.norm(v.numpy().astype(np.float64), axis=1)
        assert np.abs(n - 1.0).max() <= np.finfo(np.float32).eps
    a, b = small.numpy(), plain.numpy()
    assert not np.array_equal(a, b)
    key = lambda v: v[np.lexsort(v.T)]
    assert np.array_equal(key(a), key(b))                                    # a permutation of one another
    assert (a[:, 0] > 0).all() and a[:, 1].min() < -0.9 and a[:, 1].max() > 0.9          # the half-space in front, both sides
    assert np.isclose(np.degrees(np.arcsin(b[0, 2])), -24.8) and np.isclose(np.degrees(np.arcsin(b[-1, 2])), 2.0)
    assert np.isclose(np.degrees(np.arctan2(b[0, 1], b[0, 0])), -89.0)      # beam-major: beam 0, first azimuth (cell centre)
    # a wave of the tiled order is 8 beams x 8 azimuths: neighbours
    t64 = rm.lidar_directions(tile=8).numpy()[:64]
    az = np.degrees(np.arctan2(t64[:, 1], t64[:, 0]))
    assert len(np.unique(np.round(np.degrees(np.arcsin(t64[:, 2])), 3))) == 8 and az.max() - az.min() < 8 * 0.2
    # the counters do not depend on the order
    target, pred, origin, _, ref = scene("24x20x12")
    got = ray_metric_ref(pred[None], target[None], origin[None, None], b, grid_thresholds(THR_M), 20, "drop")
    assert np.array_equal(got, ref["drop"])
    with pytest.raises(ValueError):
        rm.lidar_directions(beams=0)
    with pytest.raises(ValueError):
        rm.lidar_directions(tile=0)


def test_sensor_origin():
    o = rm.sensor_origin((0.0, -25.6, -2.0), 0.2)
    assert o.dtype == torch.float32 and o.tolist() == [0.0, 128.0, 10.0]


def _pose(x, y, yaw_deg=0.0):
    c, s = np.cos(np.radians(yaw_deg)), np.sin(np.radians(yaw_deg))
    T = np.eye(4)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [x, y, 0.0]
    return T


def test_trajectory_origins():
    dims, org, vs = (64, 64, 16), (0.0, -6.4, -2.0), 0.2
    own = [0.0, 32.0, 10.0]
    straight = {f: _pose(1.0 * f, 0.0) for f in range(30)}                   # 1 m = 5 voxels per frame along x
    o = rm.trajectory_origins(straight, 3, 4, 2, org, vs, dims)
    assert o.dtype == torch.float32 and o.tolist() == [own, [10.0, 32.0, 10.0], [20.0, 32.0, 10.0], [30.0, 32.0, 10.0]]
    assert rm.trajectory_origins(straight, 3, 1, 2, org, vs, dims).tolist() == [own]
    # origins that leave the grid (x > 64 voxels = 12.8 m) are dropped; the count is of frames taken, not of origins kept
    assert rm.trajectory_origins(straight, 0, 6, 5, org, vs, dims).tolist() == [own, [25.0, 32.0, 10.0], [50.0, 32.0, 10.0]]
    # the world pose does not matter, only the relative one: the same drive, rotated and shifted in the world
    W = _pose(7.0, -3.0, 40.0)
    moved = {f: W @ T for f, T in straight.items()}
    assert np.allclose(rm.trajectory_origins(moved, 3, 4, 2, org, vs, dims).numpy(), o.numpy(), atol=1e-4)
    # missing frames are skipped and do not count; the walk ends with the last pose
    holes = {f: T for f, T in straight.items() if f not in (5, 7)}
    assert rm.trajectory_origins(holes, 3, 3, 2, org, vs, dims).tolist() == [own, [30.0, 32.0, 10.0], [40.0, 32.0, 10.0]]
    assert rm.trajectory_origins(straight, 28, 4, 1, org, vs, dims).tolist() == [own, [5.0, 32.0, 10.0]]
    # a curved drive: the car turns left by 10 degrees per frame while moving 2 m; positions in frame 0's grid
    curved, T = {}, np.eye(4)
    for f in range(6):
        curved[f] = T.copy()
        T = T @ _pose(2.0, 0.0, 10.0)
    got = rm.trajectory_origins(curved, 0, 6, 1, org, vs, dims).numpy()
    want, pos, head = [own], np.zeros(2), 0.0
    for f in range(1, 6):
        pos = pos + 2.0 * np.array([np.cos(np.radians(head)), np.sin(np.radians(head))])
        head += 10.0
        want.append([pos[0] / vs, (pos[1] + 6.4) / vs, 10.0])
    assert got.shape == (6, 3) and np.allclose(got, np.array(want), atol=1e-4) and got[5, 1] > got[1, 1] + 10      # it did turn left
    # seen from a later frame the earlier drive lies behind the grid: only its own origin and what is in front
    back = rm.trajectory_origins(curved, 2, 4, 1, org, vs, dims).numpy()
    assert back[0].tolist() == own and len(back) == 4 and np.allclose(back[1], [10.0, 32.0, 10.0], atol=1e-4)
    with pytest.raises(KeyError):
        rm.trajectory_origins(straight, 99, 2, 1, org, vs, dims)
    with pytest.raises(ValueError):
        rm.trajectory_origins(straight, 0, 0, 1, org, vs, dims)


# ----------------------------------------------------------------------------------------------------- the kernel stand-in
class RayStandIn:
    """hip.ray_metric on CPU tensors, from what the host side hands over (the style of tests/test_map.py's KernelStandIn
    and tests/test_visibility.py's WeightedStandIn)."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "ray_metric", self.ray_metric)
        return self

    @staticmethod
    def _volume(t):
        assert t.dim() == 4 and t.is_contiguous() and t.dtype in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16))
        a = t.numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a

    def ray_metric(self, pred, target, origins, dirs, counts, thresholds, n_classes, unknown_mode=hip.RAY_UNKNOWN_DROP):
        assert origins.dtype == torch.float32 and origins.dim() == 3 and origins.shape[0] == pred.shape[0] and origins.is_contiguous()
        assert dirs.dtype == torch.float32 and dirs.dim() == 2 and dirs.is_contiguous()
        assert counts.dtype == torch.int64 and counts.numel() == hip.ray_metric_size(n_classes, len(thresholds))
        assert all(isinstance(t, float) and np.float32(t) == t for t in thresholds)
        mode = {hip.RAY_UNKNOWN_DROP: "drop", hip.RAY_UNKNOWN_PASS: "pass"}[unknown_mode]
        self.calls.append({"batch": int(pred.shape[0]), "origins": origins.clone(), "mode": mode, "thresholds": list(thresholds),
                           "dtypes": (pred.dtype, target.dtype), "pred": pred.clone()})
        counts += torch.from_numpy(ray_metric_ref(self._volume(pred), self._volume(target), origins.numpy(), dirs.numpy(),
                                                  thresholds, n_classes, mode))
        return counts


def test_ray_metrics_on_the_stand_in_equals_the_restatement(monkeypatch):
    k = RayStandIn().install(monkeypatch)
    ta, pa, origin, dirs, ref = scene("24x20x12")
    tb = make_scene((24, 20, 12), 11)
    pb = make_prediction(tb, 11)
    C = 20
    for mode in ("drop", "pass"):
        m = rm.RayMetrics(C, KITTI_VOXEL, dirs, unknown=mode)
        assert m.counts().tolist() == [0] * m.size and m.size == 4 + 2 * C + 3 * C + 3
        assert m.add_batch(torch.from_numpy(pa[None].copy()), torch.from_numpy(ta[None].copy()), torch.from_numpy(origin.copy())) is m
        assert np.array_equal(m.counts().numpy(), ref[mode])
        # a second batch of two frames, wider labels narrowed, (K, 3) origins for all frames: the counters accumulate
        preds, targets = np.stack([pb, pa]), np.stack([tb, ta])
        origins = np.stack([origin, origin + np.float32(1.5)])
        m.add_batch(torch.from_numpy(preds.astype(np.int64)), torch.from_numpy(targets.astype(np.int32)), torch.from_numpy(origins))
        assert k.calls[-1]["dtypes"] == (torch.int16, torch.int16) and tuple(k.calls[-1]["origins"].shape) == (2, 2, 3)
        second = ray_metric_ref(preds, targets, np.broadcast_to(origins, (2, 2, 3)), dirs, grid_thresholds(THR_M), C, mode)
        assert np.array_equal(m.counts().numpy(), ref[mode] + second)
        assert k.calls[-1]["mode"] == mode and k.calls[-1]["thresholds"] == [5.0, 10.0, 20.0]
        # statistics: the arithmetic restated
        s, c = m.get_stats(), split(ref[mode] + second, C, 3)
        assert (s["rays"], s["valid"], s["unknown"], s["pred_miss"]) == (c.rays, c.valid, c.unknown, c.pred_miss)
        for t in range(3):
            for cl in range(C):
                den = c.gt[cl] + c.pred[cl] - c.tp[t, cl]
                assert s["ray_iou"][t, cl] == (c.tp[t, cl] / den if den else 0.0)
            seen = [cl for cl in range(1, C) if c.gt[cl] + c.pred[cl] > 0]
            assert np.isclose(s["ray_miou"][t], np.mean([s["ray_iou"][t, cl] for cl in seen]), rtol=1e-14, atol=0) and len(seen) >= 10
            assert s["ray_iou_geo"][t] == c.tp_geo[t] / (c.valid + (c.valid - c.pred_miss) - c.tp_geo[t])
        assert s["RayIoU"] == float(np.mean(s["ray_miou"])) and 0.0 < s["RayIoU"] < 1.0 and s["thresholds_m"] == THR_M
        # merge_ and reset
        other = rm.RayMetrics(C, KITTI_VOXEL, dirs, unknown=mode)
        other.add_batch(torch.from_numpy(pa[None].copy()), torch.from_numpy(ta[None].copy()), torch.from_numpy(origin.copy())[None, None])
        before = m.counts().clone()
        assert m.merge_(other) is m and torch.equal(m.counts(), before + other.counts())
        m.merge_(other.counts())
        assert torch.equal(m.counts(), before + 2 * other.counts())
        assert m.reset() is m and not m.counts().any()
        with pytest.raises(ValueError):
            m.merge_(torch.zeros(5, dtype=torch.int64))


def test_empty_classes_are_left_out_of_the_mean():
    C, T = 5, 2
    m = rm.RayMetrics(C, KITTI_VOXEL, PLUS_X, thresholds_m=(1.0, 2.0))
    counts = np.zeros(m.size, dtype=np.int64)
    c = split(counts, C, T)                                                  # views into counts
    counts[0:4] = [100, 60, 7, 10]
    c.gt[:] = [0, 30, 30, 0, 0]
    c.pred[:] = [0, 20, 20, 10, 0]                                           # class 3 is predicted, never true; class 4 never occurs
    c.tp[:] = [[0, 10, 20, 0, 0], [0, 20, 20, 0, 0]]
    c.tp_geo[:] = [40, 50]
    s = m.merge_(torch.from_numpy(counts)).get_stats()
    assert np.allclose(s["ray_iou"], [[0, 10 / 40, 20 / 30, 0, 0], [0, 20 / 30, 20 / 30, 0, 0]])
    assert np.allclose(s["ray_miou"], [(10 / 40 + 20 / 30 + 0) / 3, (20 / 30 + 20 / 30 + 0) / 3])      # over 1, 2, 3; 4 is excluded
    assert np.allclose(s["ray_iou_geo"], [40 / (60 + 50 - 40), 50 / (60 + 50 - 50)])
    assert np.isclose(s["RayIoU"], np.mean(s["ray_miou"]))
    empty = rm.RayMetrics(C, KITTI_VOXEL, PLUS_X).get_stats()
    assert empty["RayIoU"] == 0.0 and empty["rays"] == 0 and not empty["ray_iou_geo"].any()


def test_refusals():
    with pytest.raises(ValueError, match="n_classes"):
        rm.RayMetrics(33, 0.2, PLUS_X)
    with pytest.raises(ValueError, match="thresholds"):
        rm.RayMetrics(20, 0.2, PLUS_X, thresholds_m=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="thresholds"):
        rm.RayMetrics(20, 0.2, PLUS_X, thresholds_m=())
    with pytest.raises(ValueError, match="unknown"):
        rm.RayMetrics(20, 0.2, PLUS_X, unknown="keep")
    with pytest.raises(ValueError, match="dirs"):
        rm.RayMetrics(20, 0.2, np.zeros((4, 2), np.float32))
    m = rm.RayMetrics(20, 0.2, PLUS_X)
    lab = torch.zeros((1, 4, 3, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="integer"):
        m.add_batch(lab.float(), lab, torch.zeros(3))
    with pytest.raises(ValueError, match="shape"):
        m.add_batch(lab, lab[:, :2], torch.zeros(3))
    with pytest.raises(ValueError, match="origins"):
        m.add_batch(lab, lab, torch.zeros((2, 1, 3)))
    with pytest.raises(RuntimeError, match="GPU"):                           # no CPU path behind the binding
        m.add_batch(lab, lab, torch.zeros(3))
    counts = torch.zeros(hip.ray_metric_size(20, 3), dtype=torch.int64)
    o, d = torch.zeros((1, 1, 3)), torch.zeros((5, 3))
    with pytest.raises(RuntimeError, match="B, X, Y, Z"):
        hip.ray_metric(lab[0], lab[0], o, d, counts, (5.0, 10.0, 20.0), 20)
    with pytest.raises(RuntimeError, match="origins"):
        hip.ray_metric(lab, lab, o[0], d, counts, (5.0, 10.0, 20.0), 20)
    with pytest.raises(RuntimeError, match="dirs"):
        hip.ray_metric(lab, lab, o, d.double(), counts, (5.0, 10.0, 20.0), 20)
    with pytest.raises(RuntimeError, match="counters"):
        hip.ray_metric(lab, lab, o, d, counts[:-1], (5.0, 10.0, 20.0), 20)
    with pytest.raises(RuntimeError, match="thresholds"):
        hip.ray_metric(lab, lab, o, d, counts, (1.0,) * 5, 20)


# ----------------------------------------------------------------------------------------------------- the model hook
HOOK_FAN = {"beams": 6, "azimuth_step_deg": 15.0, "pitch_deg": (-30.0, 10.0)}


def _install(monkeypatch):
    k = RayStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    return k


def _ray_stub(**extra):
    from occdepth_amd.models.OccDepth import OccDepth
    stub = _hook_stub(**extra)
    stub._ray_epoch_end = lambda step_type: OccDepth._ray_epoch_end(stub, step_type)
    return stub


def _epoch(stub, step_type, steps, fused=None):
    """What step() and the epoch end do with the ordinary metric and the ray pass."""
    from occdepth_amd.models.OccDepth import OccDepth
    metric = getattr(stub, step_type + "_metrics")
    for n, (batch, logits, target) in enumerate(steps):
        metric.add_batch_logits(logits, target)
        if getattr(stub, "ray_metrics", None) is not None:
            OccDepth._ray_step(stub, step_type, batch, logits, target, None if fused is None else fused[n])
    (OccDepth.validation_epoch_end if step_type == "val" else OccDepth.test_epoch_end)(stub, [])


def _hook_reference(steps, origins_of, fan=HOOK_FAN, mode="drop", labels=None):
    dirs = rm.lidar_directions(**fan).numpy()
    total = 0
    for n, (batch, logits, target) in enumerate(steps):
        for i in range(len(batch["frame_id"])):
            pred = logits[i].argmax(0).numpy() if labels is None else labels[n][i].numpy()
            total = total + ray_metric_ref(pred[None], target[i].numpy()[None], origins_of(batch, i)[None], dirs,
                                           grid_thresholds(THR_M), HOOK_C, mode)
    return total


def test_model_hook_logs_and_prints(monkeypatch, tmp_path, capsys):
    from occdepth_amd.models.OccDepth import OccDepth
    k = _install(monkeypatch)
    steps = _hook_steps()
    own = rm.sensor_origin(HOOK_ORIGIN, 0.2).numpy()

    # off: a stub WITHOUT the attribute, as the existing hook tests build it -- no key, no line, no launch
    plain = _hook_stub()
    _epoch(plain, "val", steps)
    capsys.readouterr()
    _epoch(plain, "test", steps)
    lines_off = capsys.readouterr().out.splitlines()
    assert not k.calls and not any("ray" in key.lower() for key in plain.logged_keys) and not any("ray" in l for l in lines_off)

    stub = _ray_stub(ray_metrics=None)
    assert OccDepth.enable_ray_metrics(stub, **HOOK_FAN) is stub
    assert stub.ray_metrics["thresholds_m"] == (1.0, 2.0, 4.0) and stub.ray_metrics["unknown"] == "drop"
    _epoch(stub, "val", steps)
    new = set(stub.logged_keys) - set(plain.logged_keys)
    assert new == {"val_ray/RayIoU", "val_ray/RayIoU@1", "val_ray/RayIoU@2", "val_ray/RayIoU@4", "val_ray/RayIoU_geo"}
    assert all(np.array_equal(stub.logged_keys[key], plain.logged_keys[key]) for key in plain.logged_keys)
    assert [c["batch"] for c in k.calls] == [2, 1, 1] and all(tuple(c["origins"].shape[1:]) == (1, 3) for c in k.calls)
    assert all(np.array_equal(c["origins"][0, 0].numpy(), own) for c in k.calls) and all(c["mode"] == "drop" for c in k.calls)
    want = _hook_reference(steps, lambda batch, i: own[None])
    ref = rm.RayMetrics(HOOK_C, 0.2, rm.lidar_directions(**HOOK_FAN)).merge_(torch.from_numpy(want)).get_stats()
    assert ref["valid"] > 0 and stub.logged_keys["val_ray/RayIoU"] == ref["RayIoU"]
    assert stub.logged_keys["val_ray/RayIoU@2"] == ref["ray_miou"][1] and stub.logged_keys["val_ray/RayIoU_geo"] == ref["ray_iou_geo"].mean()
    assert not stub.ray_metrics["metrics"]["val"].counts().any()            # reset for the next epoch

    capsys.readouterr()
    _epoch(stub, "test", steps)
    lines = capsys.readouterr().out.splitlines()
    assert lines[:len(lines_off)] == lines_off
    block = lines[len(lines_off):]
    assert block[0] == "test_ray======" and block[1].startswith("RayIoU=%.4f, RayIoU@1=" % (ref["RayIoU"] * 100))
    assert "RayIoU_geo=" in block[1] and block[2].startswith("class RayIoU: ['0', '1', '2', '3']")
    assert [l.split(":")[0] for l in block[3:6]] == ["@1m", "@2m", "@4m"]
    assert block[6] == "rays=%d, valid=%d, unknown=%d, pred_miss=%d" % (ref["rays"], ref["valid"], ref["unknown"], ref["pred_miss"])
    assert len(block) == 7

    # the fused labels go into a second metric
    fused = [torch.roll(logits.argmax(1), 1, dims=1).to(torch.uint8) for _, logits, _ in steps]
    both = OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), unknown="pass", thresholds_m=(1, 2, 4), **HOOK_FAN)
    k.calls.clear()
    _epoch(both, "val", steps, fused)
    assert len(k.calls) == 6 and all(c["mode"] == "pass" for c in k.calls)
    assert {key for key in both.logged_keys if "fused_ray" in key} == {"val_fused_ray/RayIoU", "val_fused_ray/RayIoU@1",
            "val_fused_ray/RayIoU@2", "val_fused_ray/RayIoU@4", "val_fused_ray/RayIoU_geo"}
    want_f = _hook_reference(steps, lambda batch, i: own[None], mode="pass", labels=fused)
    ref_f = rm.RayMetrics(HOOK_C, 0.2, PLUS_X).merge_(torch.from_numpy(want_f)).get_stats()
    assert both.logged_keys["val_fused_ray/RayIoU"] == ref_f["RayIoU"] != both.logged_keys["val_ray/RayIoU"]
    capsys.readouterr()
    _epoch(both, "test", steps, fused)
    out = capsys.readouterr().out.splitlines()
    assert out.count("test_ray======") == 1 and out.count("test_fused_ray======") == 1

    # more than one origin: the later sensor positions of the sequence, inside the grid; every pose before any launch
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"                                     # camera frame: z forward = the sensor's x
    _write_sequence(root / "08", "".join(line % (0, 0.4 * f) for f in range(3)))
    _write_sequence(root / "03", "".join(line % (0, 0.4 * f) for f in range(2)))
    multi = OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), origins=3, origin_step=1, poses_root=str(root), **HOOK_FAN)
    k.calls.clear()
    _epoch(multi, "val", steps)
    from occdepth_amd import fuse
    poses = {seq: fuse.read_kitti_poses(str(root / seq)) for seq in ("08", "03")}
    origins_of = lambda batch, i: rm.trajectory_origins(poses[batch["sequence"][i]], int(batch["frame_id"][i]), 3, 1, HOOK_ORIGIN,
                                                        0.2, HOOK_DIMS).numpy()
    assert [len(origins_of(b, i)) for b, _, _ in steps for i in range(len(b["frame_id"]))] == [3, 2, 1, 1]
    assert [tuple(c["origins"].shape[:2]) for c in k.calls] == [(1, 3), (1, 2), (1, 1), (1, 1)]       # a batch whose frames kept different numbers: one launch each
    want_m = _hook_reference(steps, origins_of)
    ref_m = rm.RayMetrics(HOOK_C, 0.2, PLUS_X).merge_(torch.from_numpy(want_m)).get_stats()
    assert multi.logged_keys["val_ray/RayIoU"] == ref_m["RayIoU"] and ref_m["rays"] > ref["rays"]
    # the train step type never reaches the pass; refusals
    with pytest.raises(ValueError, match="poses_root"):
        OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), origins=2)
    with pytest.raises(NotImplementedError, match="SemanticKITTI"):
        OccDepth.enable_ray_metrics(_ray_stub(dataset="NYU", ray_metrics=None))
    with pytest.raises(ValueError, match="unknown"):
        OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), unknown="keep")
    with pytest.raises(ValueError, match="thresholds"):
        OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), thresholds_m=(1, 2, 3, 4, 5))
    gone = OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), origins=2, poses_root=str(root), **HOOK_FAN)
    k.calls.clear()
    late = ({"sequence": ["03"], "frame_id": ["000007"]}, steps[0][1][:1], steps[0][2][:1])
    with pytest.raises(KeyError, match="no pose for frame 7"):
        OccDepth._ray_step(gone, "val", *late)
    assert not k.calls


def test_allreduce_sums_the_counters_over_the_ranks(monkeypatch):
    from occdepth_amd.models.OccDepth import OccDepth
    _install(monkeypatch)
    steps = _hook_steps()

    class TwoRanks:                                                          # every rank brings what this one counted
        ReduceOp = SimpleNamespace(SUM="sum")
        calls = 0

        @staticmethod
        def is_initialized():
            return True

        @staticmethod
        def get_world_size():
            return 2

        @classmethod
        def all_reduce(cls, t, op=None):
            cls.calls += 1
            t *= 2

    m = rm.RayMetrics(HOOK_C, 0.2, rm.lidar_directions(**HOOK_FAN))
    m.merge_(torch.arange(m.size, dtype=torch.int64))
    assert m.allreduce_(TwoRanks) is m and torch.equal(m.counts(), 2 * torch.arange(m.size)) and TwoRanks.calls == 1
    # the hook asks for it only under metrics_allreduce
    seen = []
    monkeypatch.setattr(rm.RayMetrics, "allreduce_", lambda self, dist=None: seen.append(self) or self)
    for flag in (False, True):
        stub = OccDepth.enable_ray_metrics(_ray_stub(ray_metrics=None), **HOOK_FAN)
        stub.metrics_allreduce = flag
        _epoch(stub, "val", steps)
        assert len(seen) == int(flag)


def test_ray_metrics_are_switched_by_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def state():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg).ray_metrics

    for var in ("OCCDEPTH_RAY_METRIC", "OCCDEPTH_RAY_ORIGINS", "OCCDEPTH_RAY_POSES", "OCCDEPTH_RAY_UNKNOWN", "OCCDEPTH_FUSE",
                "OCCDEPTH_FUSE_POSES", "OCCDEPTH_MAP_DIR"):
        monkeypatch.delenv(var, raising=False)
    assert state() is None
    monkeypatch.setenv("OCCDEPTH_RAY_METRIC", "1")
    st = state()
    assert (st["origins"], st["origin_step"], st["unknown"], st["poses_root"], st["thresholds_m"]) == (1, 5, "drop", None, (1.0, 2.0, 4.0))
    monkeypatch.setenv("OCCDEPTH_RAY_UNKNOWN", "pass")
    monkeypatch.setenv("OCCDEPTH_RAY_ORIGINS", "4")
    with pytest.raises(ValueError, match="OCCDEPTH_RAY_POSES"):
        state()
    monkeypatch.setenv("OCCDEPTH_FUSE_POSES", str(tmp_path / "fuse"))
    st = state()
    assert (st["origins"], st["origin_step"], st["unknown"], st["poses_root"]) == (4, 5, "pass", str(tmp_path / "fuse"))
    monkeypatch.setenv("OCCDEPTH_RAY_POSES", str(tmp_path / "seq"))
    monkeypatch.setenv("OCCDEPTH_RAY_ORIGINS", "8,10")
    st = state()
    assert (st["origins"], st["origin_step"], st["poses_root"]) == (8, 10, str(tmp_path / "seq"))
    monkeypatch.setenv("OCCDEPTH_RAY_ORIGINS", "8,x")
    with pytest.raises(ValueError, match="OCCDEPTH_RAY_ORIGINS"):
        state()


def test_off_imports_nothing():
    """With the feature off the model module does not import occdepth_amd.ray_metric (checked in a fresh interpreter)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import occdepth_amd.models.OccDepth; "
            "assert 'occdepth_amd.ray_metric' not in sys.modules; print('clean')" % root)
    env = {k: v for k, v in os.environ.items() if not k.startswith("OCCDEPTH_RAY")}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "clean", out.stderr


# ----------------------------------------------------------------------------------------------------- the offline tool
def _tool():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "ray_metric.py")
    spec = importlib.util.spec_from_file_location("ray_metric_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ray_metric_tool_scores_submission_labels(monkeypatch, tmp_path, capsys):
    import pickle
    from occdepth_amd import fuse, output
    tool = _tool()
    k = _install(monkeypatch)
    dims, C = (24, 20, 12), 20
    origin = kitti_origin(dims)
    ids = np.array(output.KITTI_LEARNING_MAP_INV, dtype=np.uint16)
    pred_dir, gt_dir = tmp_path / "predictions", tmp_path / "gt"
    os.makedirs(pred_dir)
    os.makedirs(gt_dir)
    frames = []
    for n in range(3):
        target = make_scene(dims, 20 + n)
        pred = make_prediction(target, 20 + n)
        frames.append((pred, target))
        ids[pred.reshape(-1)].tofile(str(pred_dir / ("%06d.label" % n)))     # the project's submission format
        with open(gt_dir / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"target": target.astype(np.uint16)}, f)
    ids[frames[0][0].reshape(-1)].tofile(str(pred_dir / "000009.label"))     # no target for it: not scored
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    seq = _write_sequence(tmp_path / "08", "".join(line % (0, 0.6 * f) for f in range(3)))
    base = ["--pred", str(pred_dir), "--gt", str(gt_dir), "--dims", "24", "20", "12", "--origin"] + [str(o) for o in origin] + [
        "--beams", "8", "--azimuth-step", "4"]
    args = tool.parser().parse_args(base)
    assert (args.unknown, args.origins, args.classes, tuple(args.thresholds)) == ("drop", 1, 20, (1.0, 2.0, 4.0))
    stats = tool.run(args, device=torch.device("cpu"))
    dirs = rm.lidar_directions(beams=8, azimuth_step_deg=4.0).numpy()
    own = rm.sensor_origin(origin, 0.2).numpy()
    want = sum(ray_metric_ref(p[None], t[None], own[None, None], dirs, grid_thresholds(THR_M), C, "drop") for p, t in frames)
    ref = rm.RayMetrics(C, 0.2, dirs).merge_(torch.from_numpy(want)).get_stats()
    assert len(k.calls) == 3 and stats["RayIoU"] == ref["RayIoU"] and stats["valid"] == ref["valid"] > 0 and stats["unknown"] > 0
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "3 frames, 360 rays per origin" and out[1] == "ray======" and out[-1].startswith("rays=1080, valid=")
    # the same options as the hook: pass mode, thresholds, several origins from the poses
    more = tool.run(tool.parser().parse_args(base + ["--unknown", "pass", "--thresholds", "0.5", "3", "--origins", "2", "--origin-step",
                                                     "1", "--poses", seq, "--beam-major"]), device=torch.device("cpu"))
    poses = fuse.read_kitti_poses(seq)
    plain = rm.lidar_directions(beams=8, azimuth_step_deg=4.0, tile=None).numpy()
    want = sum(ray_metric_ref(p[None], t[None], rm.trajectory_origins(poses, n, 2, 1, origin, 0.2, dims).numpy()[None], plain,
                              grid_thresholds((0.5, 3.0)), C, "pass") for n, (p, t) in enumerate(frames))
    ref = rm.RayMetrics(C, 0.2, plain, thresholds_m=(0.5, 3.0)).merge_(torch.from_numpy(want)).get_stats()
    assert more["rays"] == 360 * 5 and more["unknown"] == 0 and more["RayIoU"] == ref["RayIoU"] and more["thresholds_m"] == (0.5, 3.0)
    with pytest.raises(ValueError, match="--poses"):
        tool.run(tool.parser().parse_args(base + ["--origins", "2"]), device=torch.device("cpu"))


# ----------------------------------------------------------------------------------------------------- argument checks
def test_entry_point_validates_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected

    def args():
        a = hip.RayMetricArgs()
        a.pred = a.target = a.origins = a.dirs = a.counts = ptr
        a.batch, a.n_origins, a.n_rays, a.X, a.Y, a.Z = 2, 3, 1440, 40, 24, 20
        a.pred_bytes, a.target_bytes, a.n_classes, a.n_thresholds, a.unknown_mode = 1, 2, 20, 3, 0
        a.thresholds[0], a.thresholds[1], a.thresholds[2] = 5.0, 10.0, 20.0
        return a

    fn = hip_lib.occd_ray_metric
    assert fn(None, None) == -1
    for field, value in (("pred", None), ("target", None), ("origins", None), ("dirs", None), ("counts", None), ("batch", 0),
                         ("n_origins", 0), ("n_rays", -1), ("X", 0), ("Y", -2), ("Z", 0), ("pred_bytes", 0), ("pred_bytes", 3),
                         ("pred_bytes", 4), ("target_bytes", 0), ("target_bytes", 4), ("n_thresholds", 0), ("n_thresholds", 5),
                         ("n_classes", 0), ("n_classes", 33), ("unknown_mode", 2), ("unknown_mode", -1)):
        a = args()
        setattr(a, field, value)
        assert fn(ctypes.byref(a), None) == -1, (field, value)
    a = args()
    a.X, a.Y, a.Z = 1 << 11, 1 << 10, 1 << 10                               # X Y Z = 2^31
    assert fn(ctypes.byref(a), None) == -1
    a = args()
    a.X, a.Y, a.Z = 1 << 16, 1 << 16, 1 << 16                               # X Y alone is past it
    assert fn(ctypes.byref(a), None) == -1
    a = args()
    a.batch, a.n_origins, a.n_rays = 1 << 10, 1 << 10, 1 << 11              # B K N = 2^31
    assert fn(ctypes.byref(a), None) == -1
    a = args()
    a.batch, a.n_origins, a.n_rays = 1 << 16, 1 << 16, 1
    assert fn(ctypes.byref(a), None) == -1
    # additive: the ABI version did not move, the struct is what the header says
    assert hip.ABI_VERSION == 22 and "occd_ray_metric" in hip.EXPORTS
    assert ctypes.sizeof(hip.RayMetricArgs) == 5 * 8 + 11 * 4 + 4 * 4 + 4    # 5 pointers, 11 ints, 4 floats, tail padding
    assert (hip.RAY_MAX_THRESHOLDS, hip.RAY_MAX_CLASSES, hip.RAY_COUNTERS) == (4, 32, 4)
    assert hip.ray_metric_size(20, 3) == 4 + 40 + 60 + 3
