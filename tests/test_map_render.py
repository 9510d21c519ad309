"""CPU: rendering the sequence map (K31, csrc/map_render.hip) -- `map_cast_ref`, the numpy restatement of the two-level
walk in float32 (voxel steps inside present bricks, one step over an absent brick, t_max), held to `cast_ref` of
tests/test_render.py on the densified window with exact equality of hit, face and depth bits on every ray;
semantic_map.MapVolume on a stand-in for the map kernels; the map views; the model hook and the offline tool with the
render kernel replaced by the restatement; and the argument checks of occd_map_render before any launch.
tests/test_map_render_gpu.py holds the kernel to the same restatement and to occd_render_voxels."""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from occdepth_amd import hip, render
from occdepth_amd import semantic_map as sm
from test_map import (GRIDS, HOOK_C, KernelStandIn, MapRef, V, _confusion_stand_in, _epoch, _hook_steps, _hook_stub, _tool,
                      _write_sequence, frames_for, pose, sequence)
from test_render import cast_ref, colour_ref, decode_png, kitti_calibration, rays

B = 16
BV = B ** 3
F = np.float32


# ----------------------------------------------------------------------------------------------------- restatement
def densify(rows, row_of_cell, fill=255):
    """(n, 4096) brick rows + the (Gx, Gy, Gz) directory of ALL rows -> the dense (16 Gx, 16 Gy, 16 Gz) uint8 volume in
    which absent bricks hold `fill`."""
    G = row_of_cell.shape
    dense = np.full((G[0] * B, G[1] * B, G[2] * B), fill, dtype=np.uint8)
    for c in zip(*np.nonzero(row_of_cell >= 0)):
        dense[c[0] * B:(c[0] + 1) * B, c[1] * B:(c[1] + 1) * B, c[2] * B:(c[2] + 1) * B] = \
            np.asarray(rows[row_of_cell[c]]).reshape(B, B, B)
    return dense


def dense_to_sparse_hit(hit, row_of_cell):
    """Linear voxel index of the dense window (or -1) -> row * 4096 + brick-local index (or -1)."""
    G = row_of_cell.shape
    h = np.maximum(hit.astype(np.int64), 0)
    Y, Z = G[1] * B, G[2] * B
    ix, iy, iz = h // (Y * Z), (h // Z) % Y, h % Z
    row = row_of_cell[ix >> 4, iy >> 4, iz >> 4].astype(np.int64)
    out = row * BV + (((ix & 15) * B + (iy & 15)) * B + (iz & 15))
    assert (row[hit >= 0] >= 0).all()
    return np.where(hit >= 0, out, -1)


def map_cast_ref(labels, cells, origin, dirs, target=None, t_max=np.inf, skip=True):
    """The walk of csrc/map_render.hip in float32, ray by ray in lockstep -> hit (row * 4096 + local or -1, int64), face,
    depth, and the counters {"skipped": per-ray bool (left at least one absent brick in one step), "up", "down": single
    correction steps of the skip, "started_absent": rays whose first voxel lies in an absent brick, "iterations"}."""
    G = np.array(cells.shape, dtype=np.int64)
    idims = G * B
    dims = idims.astype(F)
    shape = origin.shape[:-1]
    o = np.ascontiguousarray(origin.reshape(-1, 3).astype(F))
    d = np.ascontiguousarray(dirs.reshape(-1, 3).astype(F))
    n = o.shape[0]
    cflat = np.asarray(cells).reshape(-1).astype(np.int64)
    n_rows = labels.shape[0]
    flat = np.asarray(labels).reshape(-1).astype(np.int64)
    tflat = None if target is None else np.asarray(target).reshape(-1).astype(np.int64)
    inf, tmax = F(np.inf), F(t_max)
    stats = {"skipped": np.zeros(n, dtype=bool), "up": 0, "down": 0, "started_absent": 0, "iterations": 0}
    with np.errstate(all="ignore"):
        alive = np.isfinite(o).all(1) & np.isfinite(d).all(1)
        nz = d != 0
        inv = np.where(nz, F(1) / np.where(nz, d, F(1)), F(0)).astype(F)
        tn, tf, axis = np.full(n, -inf, F), np.full(n, inf, F), np.full(n, 3)
        for a in range(3):
            ta, tc = (F(0) - o[:, a]) * inv[:, a], (dims[a] - o[:, a]) * inv[:, a]
            lo, hi = np.fmin(ta, tc), np.fmax(ta, tc)
            upd = nz[:, a] & (lo > tn)
            tn, axis = np.where(upd, lo, tn), np.where(upd, a, axis)
            tf = np.where(nz[:, a], np.fmin(tf, hi), tf)
            alive &= nz[:, a] | ((o[:, a] >= 0) & (o[:, a] < dims[a]))
        entered = tn > 0
        t = np.where(entered, tn, F(0)).astype(F)
        face = np.where(entered, axis, 3)
        alive &= tf >= t
        idx = np.fmin(np.fmax(np.floor(o + d * t[:, None]), F(0)), dims - F(1))
        idx = np.where(np.isfinite(idx), idx, 0).astype(np.int64)
        step = np.sign(d).astype(np.int64)
        up = (step > 0).astype(np.int64)

        def bound(i, sel):
            """m_a(i) of the rays `sel`, +inf on an axis the ray does not move along."""
            return np.where(step[sel] != 0, ((i + up[sel]).astype(F) - o[sel]) * inv[sel], inf).astype(F)

        m = bound(idx, slice(None))
        hit = np.full(n, -1, dtype=np.int64)

        def voxel_step(act):
            mm = m[act]
            ax = np.where((mm[:, 0] <= mm[:, 1]) & (mm[:, 0] <= mm[:, 2]), 0, np.where(mm[:, 1] <= mm[:, 2], 1, 2))
            mv = mm[np.arange(act.size), ax]
            go = (mv < inf) & ~(mv > tmax)
            alive[act[~go]] = False
            act, ax, mv = act[go], ax[go], mv[go]
            idx[act, ax] += step[act, ax]
            ok = (idx[act, ax] >= 0) & (idx[act, ax] < idims[ax])
            alive[act[~ok]] = False
            act, ax, mv = act[ok], ax[ok], mv[ok]
            face[act], t[act] = ax, mv
            m[act, ax] = ((idx[act, ax] + up[act, ax]).astype(F) - o[act, ax]) * inv[act, ax]

        def brick_step(act):
            i, s = idx[act], step[act]
            last = np.where(s > 0, i | (B - 1), i & ~(B - 1))
            M = bound(last, act)
            ax = np.where((M[:, 0] <= M[:, 1]) & (M[:, 0] <= M[:, 2]), 0, np.where(M[:, 1] <= M[:, 2], 1, 2))
            Mv = M[np.arange(act.size), ax]
            go = (Mv < inf) & ~(Mv > tmax)
            alive[act[~go]] = False
            act, i, s, last, ax, Mv = act[go], i[go], s[go], last[go], ax[go], Mv[go]
            new = i.copy()
            for b in range(3):
                r = np.nonzero((ax != b) & (s[:, b] != 0))[0]
                ib, sb, lb, ub = i[r, b], s[r, b], last[r, b], up[act[r], b]
                ob, db, nb, Mb = o[act[r], b], d[act[r], b], inv[act[r], b], Mv[r]
                e = np.fmin(np.fmax(np.floor(ob + db * Mb), np.minimum(ib, lb).astype(F)), np.maximum(ib, lb).astype(F))
                e = e.astype(np.int64)
                first = b < ax[r]                                  # b wins a tie against the exit axis

                def precedes(j):
                    mj = ((j + ub).astype(F) - ob) * nb
                    return np.where(first, mj <= Mb, mj < Mb)
                while True:
                    c = (e != ib) & ~precedes(e - sb)
                    if not c.any():
                        break
                    e = np.where(c, e - sb, e)
                    stats["down"] += int(c.sum())
                while True:
                    c = (e != lb) & precedes(e)
                    if not c.any():
                        break
                    e = np.where(c, e + sb, e)
                    stats["up"] += int(c.sum())
                new[r, b] = e
            k = np.arange(act.size)
            new[k, ax] = last[k, ax] + s[k, ax]
            stats["skipped"][act] = True
            ok = (new[k, ax] >= 0) & (new[k, ax] < idims[ax])
            alive[act[~ok]] = False
            act, new, ax, Mv = act[ok], new[ok], ax[ok], Mv[ok]
            idx[act] = new
            face[act], t[act] = ax, Mv
            m[act] = bound(new, act)

        for it in range(B * int(G.sum()) + 3):
            act = np.nonzero(alive)[0]
            if act.size == 0:
                break
            stats["iterations"] += int(act.size)
            i = idx[act]
            row = cflat[((i[:, 0] >> 4) * G[1] + (i[:, 1] >> 4)) * G[2] + (i[:, 2] >> 4)]
            row = np.where(row >= n_rows, -1, row)
            present = row >= 0
            if it == 0:
                stats["started_absent"] = int((~present).sum())
            at = np.where(present, row, 0) * BV + (((i[:, 0] & 15) * B + (i[:, 1] & 15)) * B + (i[:, 2] & 15))
            lab = flat[at]
            occ = (lab > 0) & (lab < 255)
            vis = present & (occ if tflat is None else (tflat[at] != 255) & (occ | (tflat[at] != 0)))
            good = vis & (t[act] <= tmax)
            hit[act[good]] = at[good]
            alive[act[vis]] = False
            walk = (present & ~vis) | (~present & (not skip))
            voxel_step(act[walk])
            if skip:
                brick_step(act[~present])
        assert not alive.any(), "the iteration bound was reached"
    miss = hit < 0
    return (hit.reshape(shape), np.where(miss, 3, face).reshape(shape).astype(np.uint8),
            np.where(miss, inf, t).reshape(shape).astype(F), stats)


def with_t_max(dense_result, t_max):
    """(hit, face, depth) of the dense walk with every hit of depth > t_max turned into a miss."""
    hit, face, depth = dense_result
    far = (hit >= 0) & (depth > F(t_max))
    return np.where(far, -1, hit), np.where(far, 3, face).astype(np.uint8), np.where(far, F(np.inf), depth).astype(F)


class MapRenderStandIn:
    """hip.map_render on CPU tensors: the restatement and the integer colour rule."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "map_render", self.map_render)
        return self

    def map_render(self, labels, cells, views, size, palette, target=None, background=None, alpha=256,
                   bg_colour=(255, 255, 255), view_sizes=None, t_max=float("inf"), skip=True, aux=False):
        H, W = size
        Vn = views.shape[0]
        self.calls.append({"views": Vn, "size": (H, W), "error": target is not None, "t_max": t_max})
        lab, tg = labels.numpy().reshape(-1, BV), None if target is None else target.numpy().reshape(-1, BV)
        rgb = np.empty((Vn, H, W, 3), dtype=np.uint8)
        hit, face = np.full((Vn, H, W), -1, dtype=np.int64), np.full((Vn, H, W), 3, dtype=np.uint8)
        depth = np.full((Vn, H, W), np.inf, dtype=F)
        for i in range(Vn):
            h, w = view_sizes[i] if view_sizes is not None else (H, W)
            o, d = rays(views[i].numpy(), h, w, F)
            hit[i, :h, :w], face[i, :h, :w], depth[i, :h, :w], _ = map_cast_ref(lab, cells.numpy(), o, d, tg, t_max, skip)
            back = None if background is None else background[i].numpy()
            rgb[i] = colour_ref(lab, hit[i], face[i], palette.numpy(), target=tg, background=back, alpha=alpha, bg=bg_colour)
        out = (torch.from_numpy(rgb), torch.from_numpy(hit), torch.from_numpy(face), torch.from_numpy(depth))
        return out if aux else out[0]


# ----------------------------------------------------------------------------------------------------- the hand-placed case
WINDOW_G = (4, 3, 2)
WINDOW_KEY_MIN = np.array([-2, -1, -1])
WINDOW_DIMS = tuple(B * g for g in WINDOW_G)
WINDOW_SEED = 0
WINDOW_T_MAX = 40.0                     # voxels in the orthographic views, metres x 5 = voxels in the camera's: both cut rays
N_CLASSES = 20
CAM_F = 60.0                            # pixels: a 61 x 37 picture sees 54 x 34 degrees
OBLIQUE_HW = (19, 33)
OBLIQUE_AZ, OBLIQUE_EL, OBLIQUE_ZOOM = -8.0, 15.0, 0.25   # nearly along the row of present bricks, zoomed onto it


@functools.lru_cache(maxsize=None)
def window_case(seed=WINDOW_SEED):
    """4 x 3 x 2 bricks with negative keys: about a third present, one of those with nothing drawable (labels 0 and 255,
    a target of 0 and 255), about 1 % of the voxels of the others occupied; the corner bricks of the bounding box are
    present so that the window is the whole box.  -> dict: keys (n, 3), labels / target (n, 4096), row_of_cell (every
    row), cells (the empty brick dropped), views {name: (view (18,), (H, W))}."""
    rng = np.random.RandomState(seed)
    G = WINDOW_G
    all_cells = [(a, b, c) for a in range(G[0]) for b in range(G[1]) for c in range(G[2])]
    corners = [(0, 0, 0), (G[0] - 1, G[1] - 1, G[2] - 1)]
    camera_cell = (0, 1, 0)                                              # absent: the camera starts in an absent brick
    row = [(a, 1, c) for a in (1, 2, 3) for c in (0, 1)]                 # what the camera looks down and the oblique view along
    present = sorted(corners + row)                                      # 8 of 24, ascending (k0, k1, k2)
    assert camera_cell not in present and len(set(present)) == 8 and all(c in all_cells for c in present)
    n = len(present)
    labels = np.zeros((n, BV), dtype=np.uint8)
    target = np.zeros((n, BV), dtype=np.uint8)
    for arr in (labels, target):
        occ = rng.rand(n, BV) < 0.01
        arr[occ] = rng.randint(1, N_CLASSES, size=int(occ.sum()))
        arr[rng.rand(n, BV) < 0.02] = 255
    empty = 7                                                            # this row has nothing to draw in any mode
    labels[empty] = np.where(rng.rand(BV) < 0.5, 0, 255)
    target[empty] = np.where(labels[empty] == 255, 255, 0)
    target[labels == 255] = 255                                          # MapVolume's rule
    row_of_cell = np.full(G, -1, dtype=np.int32)
    for r, c in enumerate(present):
        row_of_cell[c] = r
    cells = row_of_cell.copy()
    cells[present[empty]] = -1
    keys = np.array(present, dtype=np.int64) + WINDOW_KEY_MIN
    return {"keys": keys, "labels": labels, "target": target, "row_of_cell": row_of_cell, "cells": cells,
            "empty": empty, "views": window_views()}


def make_views(dims, cam_at):
    """The five views of the tests over a window of `dims` voxels -> {name: (view (18,) float32 numpy, (H, W))}: a camera
    at the window voxel coordinate `cam_at` looking along +x, the BEV at one pixel per voxel, an oblique view nearly
    along x zoomed onto the window's middle, exact ties, and rays with two zero direction components.  The sizes of
    camera, oblique and tie are no multiple of the kernel's 8 x 8 tile."""
    X, Y, Z = dims
    _, E = kitti_calibration(61)
    k = np.array([[CAM_F, 0.0, 30.0], [0.0, CAM_F, 18.0], [0.0, 0.0, 1.0]])
    centre = -E[:3, :3].T @ E[:3, 3]
    origin = centre - np.asarray(cam_at, dtype=np.float64) * V
    cam = render.camera_view(torch.from_numpy(k), torch.from_numpy(E), tuple(origin), V).numpy()
    obl = render.oblique_view(dims, OBLIQUE_HW, OBLIQUE_AZ, OBLIQUE_EL, device="cpu").numpy().copy()
    z = np.float32(OBLIQUE_ZOOM)
    obl[0:3] += (OBLIQUE_HW[1] / 2) * (1 - z) * obl[3:6] + (OBLIQUE_HW[0] / 2) * (1 - z) * obl[6:9]
    obl[3:9] *= z
    # integer origins (-3 + v, u, Z + 2) once the half pixel is added, direction (1, 1, -1): every crossing is a tie
    tie = np.array([-3.5, -0.5, Z + 2, 0, 1, 0, 1, 0, 0, 1, 1, -1] + [0] * 6, dtype=F)
    zero = np.array([-2, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0] + [0] * 6, dtype=F)          # along +x at half-integer (y, z)
    return {"camera": (cam, (37, 61)), "bev": (render.bev_view(dims, 1, device="cpu").numpy(), (X, Y)),
            "oblique": (obl, OBLIQUE_HW), "tie": (tie, (45, 28)), "zero": (zero, (Z, Y))}


def window_views():
    return make_views(WINDOW_DIMS, (8.5, 24.5, 9.5))                     # the camera sits in the absent brick (0, 1, 0)


@functools.lru_cache(maxsize=None)
def window_refs(mode, t_max):
    """{view: (hit, face, depth, stats)} of the restatement on the window case; computed once, never changed."""
    case = window_case()
    tg = case["target"] if mode == "error" else None
    out = {}
    for name, (view, (H, W)) in case["views"].items():
        o, d = rays(view, H, W, F)
        out[name] = map_cast_ref(case["labels"], case["cells"], o, d, tg, t_max)
    return out


@functools.lru_cache(maxsize=None)
def window_dense(mode):
    """{view: (hit mapped to row * 4096 + local, face, depth)} of cast_ref on the densified window, float32."""
    case = window_case()
    dl = densify(case["labels"], case["row_of_cell"])
    dt = densify(case["target"], case["row_of_cell"]) if mode == "error" else None
    out = {}
    for name, (view, (H, W)) in case["views"].items():
        hit, face, depth = cast_ref(dl, *rays(view, H, W, F), F, target=dt)
        out[name] = (dense_to_sparse_hit(hit, case["row_of_cell"]), face, depth)
    return out


def bits(depth):
    return np.ascontiguousarray(depth, dtype=F).view(np.int32)


@pytest.mark.parametrize("t_max", [np.inf, WINDOW_T_MAX], ids=["inf", "finite"])
@pytest.mark.parametrize("mode", ["class", "error"])
def test_restatement_equals_the_flat_walk_on_the_densified_window(mode, t_max):
    case = window_case()
    assert len(case["keys"]) == 8 and (case["keys"].min(0) < 0).all()
    density = ((case["labels"] > 0) & (case["labels"] < 255)).mean(1)
    assert density[case["empty"]] == 0 and 0.007 < np.delete(density, case["empty"]).mean() < 0.013
    refs, dense = window_refs(mode, t_max), window_dense(mode)
    up = down = started = cut = 0
    for name, (view, (H, W)) in case["views"].items():
        hit, face, depth, stats = refs[name]
        want = with_t_max(dense[name], t_max)
        cut += int(((dense[name][0] >= 0) & (want[0] < 0)).sum())
        assert np.array_equal(hit, want[0]), (name, int((hit != want[0]).sum()))
        assert np.array_equal(face, want[1]), name
        assert np.array_equal(bits(depth), bits(want[2])), name
        # walking the absent bricks voxel by voxel is the same walk
        o, d = rays(view, H, W, F)
        flat = map_cast_ref(case["labels"], case["cells"], o, d, case["target"] if mode == "error" else None, t_max, skip=False)
        assert all(np.array_equal(a, b) for a, b in zip(flat[:2], (hit, face))) and np.array_equal(bits(flat[2]), bits(depth))
        assert stats["iterations"] <= flat[3]["iterations"] and (stats["iterations"] < flat[3]["iterations"] or t_max != np.inf)
        up, down, started = up + stats["up"], down + stats["down"], started + stats["started_absent"]
        hits = hit >= 0
        share, skipped = hits.mean(), (stats["skipped"].reshape(hit.shape) & hits).sum() / max(hits.sum(), 1)
        print(f"{mode} t_max {t_max} {name} {W}x{H}: hits {share:.3f}, of which skipped {skipped:.3f}, corrections +{stats['up']} "
              f"-{stats['down']}, iterations {stats['iterations']} (voxel walk {flat[3]['iterations']})")
        if name in ("camera", "oblique") and t_max == np.inf:
            assert share >= 0.25, (name, share)
            assert skipped >= 0.1, (name, skipped)
    # not vacuous: the skip was corrected both ways, rays started in an absent brick, and a finite t_max cut hits
    assert up >= 1 and down >= 1 and started >= 1
    assert (cut > 0) == (t_max != np.inf)


def test_restatement_edge_cases():
    cells = np.full((2, 1, 1), -1, dtype=np.int32)
    cells[1, 0, 0] = 0
    rows = np.zeros((1, BV), dtype=np.uint8)
    rows[0, (3 * B + 5) * B + 7] = 9                                     # window voxel (19, 5, 7)
    f = lambda o, d, **kw: [x.item() for x in map_cast_ref(rows, cells, np.array([o], dtype=F), np.array([d], dtype=F), **kw)[:3]]
    at = (3 * B + 5) * B + 7
    assert f((-2.0, 5.5, 7.5), (1, 0, 0)) == [at, 0, 21.0]               # over the absent brick in one step, then 3 voxels
    assert f((-2.0, 5.5, 7.5), (1, 0, 0), t_max=21.0) == [at, 0, 21.0] and f((-2.0, 5.5, 7.5), (1, 0, 0), t_max=20.5)[0] == -1
    assert f((3.5, 5.5, 7.5), (0, 0, 0))[0] == -1                        # nothing to cross inside an absent brick
    assert f((3.5, 5.5, 7.5), (-1, 0, 0))[0] == -1                       # leaves the window from an absent brick
    assert f((19.5, 5.5, 7.5), (0, 0, 0)) == [at, 3, 0.0]
    assert f((13.0, -1.0, 7.5), (1, 1, 0)) == [at, 1, 6.0]               # ties all the way: x first, so the hit is entered by y
    assert f((np.nan, 5.5, 7.5), (1, 0, 0))[0] == -1


# ----------------------------------------------------------------------------------------------------- MapVolume
def _two_maps(monkeypatch, dims=(40, 24, 20), C=12):
    KernelStandIn().install(monkeypatch)
    origin = GRIDS[dims]
    maps = [sm.SemanticMap(C, V, origin, dims, chunk_bricks=8) for _ in range(2)]
    refs = [MapRef(C, origin, dims) for _ in range(2)]
    poses = sequence(dims)
    for (lab, mask), P in zip(frames_for(dims, C, 31, 3, masked=True), (poses[0], poses[3], poses[4])):     # the prediction, masked
        maps[0].integrate(torch.from_numpy(lab), P, mask=torch.from_numpy(mask))
        refs[0].integrate(lab, P, mask)
    for (lab, _), P in zip(frames_for(dims, C, 32, 3), (poses[1], poses[2], poses[5])):   # the truth: 1, 2 and the far jump
        maps[1].integrate(torch.from_numpy(lab), P)
        refs[1].integrate(lab, P)
    return maps, refs


def test_map_volume_rows_window_and_directory(monkeypatch):
    (pred, gt), (pref, gref) = _two_maps(monkeypatch)
    kp, kg = {tuple(k) for k in pred.brick_keys().tolist()}, {tuple(k) for k in gt.brick_keys().tolist()}
    assert kp - kg and kg - kp                                           # neither covers the other: the union is tested
    vol = sm.MapVolume(pred, gt, chunk_bricks=5)
    keys = [tuple(k) for k in vol.keys.tolist()]
    assert keys == sorted(kp | kg) and vol.n_rows == len(keys)
    assert vol.labels.dtype == torch.uint8 and tuple(vol.labels.shape) == (len(keys), BV) and vol.labels.is_contiguous()
    want_l = np.stack([pref.labels(k).reshape(-1) for k in keys])
    want_t = np.stack([gref.labels(k).reshape(-1) for k in keys])
    want_t = np.where(want_l == 255, 255, want_t)                        # counts only where both maps were observed
    assert np.array_equal(vol.labels.numpy(), want_l) and np.array_equal(vol.target.numpy(), want_t)
    assert (want_t[want_l != 255] != 255).any() and ((want_l == 255) & (np.stack([gref.labels(k).reshape(-1) for k in keys]) != 255)).any()
    kmin, kmax = np.array(keys).min(0), np.array(keys).max(0)
    assert np.array_equal(vol.key_min, kmin) and np.array_equal(vol.key_max, kmax) and vol.grid == tuple(kmax - kmin + 1)
    assert vol.dims == tuple(16 * g for g in vol.grid) and (kmin < 0).any()
    assert vol.origin_voxels.dtype == np.int64 and np.array_equal(vol.origin_voxels, 16 * kmin)
    assert vol.origin_metres.dtype == np.float64 and np.array_equal(vol.origin_metres, (16 * kmin) * V)
    # the directory: every key at its cell, a brick with nothing to draw dropped, -1 elsewhere
    occ_l = (want_l > 0) & (want_l < 255)
    drawable = (occ_l | ((want_t != 255) & (want_t != 0))).any(1)
    assert not drawable.all() and drawable.any()                         # over-selected bricks without a vote exist
    cells = vol.cells.numpy()
    assert cells.dtype == np.int32 and cells.shape == vol.grid
    want_c = np.full(vol.grid, -1, dtype=np.int32)
    for r, k in enumerate(keys):
        want_c[tuple(np.array(k) - kmin)] = r if drawable[r] else -1
    assert np.array_equal(cells, want_c) and (cells == -1).sum() > len(keys) - drawable.sum()
    full = sm.MapVolume(pred, gt, drop_empty=False)
    for r, k in enumerate(keys):
        want_c[tuple(np.array(k) - kmin)] = r
    assert np.array_equal(full.cells.numpy(), want_c) and torch.equal(full.labels, vol.labels)
    # without gt: the prediction's own bricks, class mode's rule
    alone = sm.MapVolume(pred)
    assert [tuple(k) for k in alone.keys.tolist()] == sorted(kp) and alone.target is None
    al = alone.labels.numpy()
    assert np.array_equal((alone.cells.numpy() >= 0).sum(), ((al > 0) & (al < 255)).any(1).sum())
    tv = vol.target_volume()
    assert tv.target is None and tv.labels is vol.target and tv.cells is vol.cells and vol.target is not None


def test_map_volume_min_obs_and_key_range(monkeypatch):
    (pred, gt), (pref, gref) = _two_maps(monkeypatch)
    vol = sm.MapVolume(pred, gt, min_obs=2, chunk_bricks=7)
    keys = [tuple(k) for k in vol.keys.tolist()]
    votes = np.stack([pref.brick(k).reshape(BV, -1).sum(-1) for k in keys])
    want_l = np.where(votes < 2, 255, np.stack([pref.labels(k).reshape(-1) for k in keys]))
    assert ((votes == 1).any() and (votes >= 2).any()) and np.array_equal(vol.labels.numpy(), want_l)
    want_t = np.where(want_l == 255, 255, np.stack([gref.labels(k).reshape(-1) for k in keys]))
    assert np.array_equal(vol.target.numpy(), want_t)
    # key_range: an inclusive box of brick keys
    allk = np.array(keys)
    lo, hi = allk.min(0) + [1, 0, 0], allk.max(0) - [1, 1, 0]
    part = sm.MapVolume(pred, gt, key_range=(lo, hi))
    inside = [k for k in keys if all(lo[a] <= k[a] <= hi[a] for a in range(3))]
    assert 0 < len(inside) < len(keys) and [tuple(k) for k in part.keys.tolist()] == inside
    assert (part.key_min >= lo).all() and (part.key_max <= hi).all()
    first = sm.MapVolume(pred, gt)
    rows = [keys.index(k) for k in inside]
    assert torch.equal(part.labels, first.labels[rows]) and torch.equal(part.target, first.target[rows])


def test_map_volume_refusals(monkeypatch):
    (pred, gt), _ = _two_maps(monkeypatch, dims=(16, 12, 8), C=5)
    with pytest.raises(ValueError, match="key_range"):
        sm.MapVolume(pred, gt, key_range=((500, 500, 500), (501, 501, 501)))      # no rows at all
    with pytest.raises(ValueError, match="key_range"):
        sm.MapVolume(sm.SemanticMap(5, V, GRIDS[(16, 12, 8)], (16, 12, 8)))       # an empty map
    far = sm.SemanticMap(5, V, GRIDS[(16, 12, 8)], (16, 12, 8))
    far.directory = {int(p): i for i, p in enumerate(sm.pack_keys([[0, 0, 0], [70000, 0, 0]]))}
    with pytest.raises(ValueError, match=r"2\^16.*key_range"):
        sm.MapVolume(far)                                                          # G above 2^16
    far.directory = {int(p): i for i, p in enumerate(sm.pack_keys([[0, 0, 0], [1023, 1023, 255]]))}
    with pytest.raises(ValueError, match=r"2\^27.*key_range"):
        sm.MapVolume(far)                                                          # 2^28 cells
    other = sm.SemanticMap(5, 0.4, GRIDS[(16, 12, 8)], (16, 12, 8))
    with pytest.raises(ValueError, match="voxel size"):
        sm.MapVolume(pred, other)
    with pytest.raises(ValueError, match="min_obs"):
        sm.MapVolume(pred, gt, min_obs=0)


# ----------------------------------------------------------------------------------------------------- views
def _volume_stub(dims, origin_voxels=(0, 0, 0), v=V):
    ov = np.asarray(origin_voxels, dtype=np.int64)
    return SimpleNamespace(dims=tuple(dims), voxel_size=v, origin_voxels=ov, origin_metres=ov.astype(np.float64) * v,
                           labels=torch.zeros(1, dtype=torch.uint8), n_classes=N_CLASSES)


def test_map_bev_view_is_first_drawable_voxel_from_the_top(monkeypatch):
    KernelStandIn().install(monkeypatch)
    MapRenderStandIn().install(monkeypatch)
    dims, C = (40, 24, 20), 12
    lab = frames_for(dims, C, 41, 1)[0][0]
    lab[5:9, 3:7, :] = 0                                                 # columns with nothing in them
    m = sm.SemanticMap(C, V, GRIDS[dims], dims).integrate(torch.from_numpy(lab), pose())
    vol = sm.MapVolume(m)
    X, Y, Z = vol.dims
    dense = densify(vol.labels.numpy(), _rows_of(vol))
    occ = (dense > 0) & (dense < 255)
    top = np.where(occ.any(2), Z - 1 - np.argmax(occ[:, :, ::-1], axis=2), -1)
    x, y = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    want = dense_to_sparse_hit(np.where(top >= 0, (x * Y + y) * Z + top, -1), _rows_of(vol))
    for max_side, ppv in ((max(X, Y), 1), (2 * max(X, Y) + 1, 2)):
        view, (h, w) = render.map_bev_view(vol, max_side)
        assert (h, w) == (X * ppv, Y * ppv) and torch.equal(view, render.bev_view(vol.dims, ppv, device="cpu"))
        rgb, hit, face, depth = render.render_map(vol, view, (h, w), return_aux=True)
        got = hit[0].numpy()[ppv // 2::ppv, ppv // 2::ppv]
        assert np.array_equal(got, want[::-1, ::-1]) and (want >= 0).mean() > 0.3 and (want < 0).any()
        assert np.array_equal(np.repeat(np.repeat(got, ppv, 0), ppv, 1), hit[0].numpy())
    assert render.map_bev_view(vol)[1] == ((2048 // max(X, Y)) * X, (2048 // max(X, Y)) * Y)
    # a window longer than max_side: one pixel per n x n columns, the one under its centre (point sampling)
    view, (h, w) = render.map_bev_view(vol, max_side=max(X, Y) // 2 + 1)
    assert (h, w) == (X // 2, Y // 2) and max(h, w) <= max(X, Y) // 2 + 1
    hit = render.render_map(vol, view, (h, w), return_aux=True)[1][0].numpy()
    assert np.array_equal(hit, want[::-1, ::-1][::2, ::2])              # the ray at x = X - 2 v - 1, y = Y - 2 u - 1
    with pytest.raises(ValueError, match="max_side"):
        render.map_bev_view(vol, 0)


def _rows_of(vol):
    """The directory of every row of a MapVolume, dropped bricks included."""
    out = np.full(vol.grid, -1, dtype=np.int32)
    at = vol.keys - vol.key_min
    out[at[:, 0], at[:, 1], at[:, 2]] = np.arange(len(at))
    return out


def test_map_camera_view_hit_points_project_back_into_their_pixel():
    """The analogue of test_render's camera test with the ego pose in between, 3 km from world zero: the point
    origin + t dir of pixel (u, v), taken to the world, then through the inverse pose and the calibration, lands in
    pixel (u, v) at depth t."""
    H, W = 37, 122
    k, E = kitti_calibration(W)
    P = pose(37.0, 1.5, (2100.0, -2140.0, 31.0))                         # 3 km away
    assert np.linalg.norm(P[:3, 3]) > 2990
    origin_voxels = 16 * np.floor(P[:3, 3] / V / 16).astype(np.int64) - [32, 48, 16]
    vol = _volume_stub((160, 160, 48), origin_voxels)
    view = render.map_camera_view(torch.from_numpy(k), torch.from_numpy(E), P, vol)
    assert view.dtype == torch.float32 and tuple(view.shape) == (18,) and np.abs(view.numpy()[:3]).max() < 100
    o, d = rays(view.numpy(), H, W, np.float64)
    Pinv = np.linalg.inv(P)
    for t in (2.5, 11.0):
        world = (o + d * t) * V + vol.origin_metres
        sensor = world @ Pinv[:3, :3].T + Pinv[:3, 3]
        cam = sensor @ E[:3, :3].T + E[:3, 3]
        px, py = cam[..., 0] * k[0, 0] / cam[..., 2] + k[0, 2], cam[..., 1] * k[1, 1] / cam[..., 2] + k[1, 2]
        uu, vv = np.meshgrid(np.arange(W), np.arange(H))
        assert np.abs(px - uu).max() < 2e-3 and np.abs(py - vv).max() < 2e-3
        assert np.array_equal(np.rint(px), uu) and np.array_equal(np.rint(py), vv)
        assert np.abs(cam[..., 2] - t).max() < 1e-4
    # it is camera_view of the composed extrinsic
    composed = render.camera_view(torch.from_numpy(k), torch.from_numpy(E @ Pinv), tuple(vol.origin_metres), V)
    assert torch.allclose(view, composed, atol=1e-4, rtol=1e-5)
    # flip mirrors the image
    flipped = render.map_camera_view(torch.from_numpy(k), torch.from_numpy(E), P, vol, flip=True, width=W)
    of, df = rays(flipped.numpy(), H, W, np.float64)
    assert np.allclose(of[:, ::-1], o, atol=1e-5) and np.allclose(df[:, ::-1], d, atol=1e-6) and not np.allclose(df, d, atol=1e-3)
    with pytest.raises(ValueError):
        render.map_camera_view(torch.from_numpy(k), torch.from_numpy(E), P, vol, flip=True)


def test_map_oblique_view_and_render_map_validation(monkeypatch):
    vol = _volume_stub((64, 48, 32))
    assert torch.equal(render.map_oblique_view(vol, (45, 60), -30.0, 20.0), render.oblique_view((64, 48, 32), (45, 60), -30.0, 20.0, device="cpu"))
    vol.target, vol.cells = None, torch.zeros((4, 3, 2), dtype=torch.int32)
    view = render.map_oblique_view(vol, (8, 8))
    with pytest.raises(ValueError, match="mode"):
        render.render_map(vol, view, (8, 8), mode="depth")
    with pytest.raises(ValueError, match="gt"):
        render.render_map(vol, view, (8, 8), mode="error")
    with pytest.raises(ValueError, match="sizes"):
        render.render_map(vol, [view, view], [(8, 8)])
    vol.labels = torch.zeros((1, BV), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        render.render_map(vol, view, (8, 8))                             # there is no CPU path
    # the canvas of per-view sizes and the crop, on the stand-in
    MapRenderStandIn().install(monkeypatch)
    case = window_case()
    vol = SimpleNamespace(labels=torch.from_numpy(case["labels"]), target=torch.from_numpy(case["target"]),
                          cells=torch.from_numpy(case["cells"]), n_classes=N_CLASSES, dims=WINDOW_DIMS)
    names = ["camera", "zero"]
    out = render.render_map(vol, [torch.from_numpy(case["views"][n][0]) for n in names], [case["views"][n][1] for n in names],
                            mode="error", return_aux=True, t_max=WINDOW_T_MAX)
    for i, n in enumerate(names):
        ref = window_refs("error", WINDOW_T_MAX)[n]
        assert tuple(out[0][i].shape) == case["views"][n][1] + (3,)
        assert np.array_equal(out[1][i].numpy(), ref[0]) and np.array_equal(out[2][i].numpy(), ref[1])


# ----------------------------------------------------------------------------------------------------- hook and tool
def _sequences(tmp_path):
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    return root


def test_model_hook_draws_the_maps_when_asked(monkeypatch, tmp_path):
    from occdepth_amd.models.OccDepth import OccDepth
    KernelStandIn().install(monkeypatch)
    draws = MapRenderStandIn().install(monkeypatch)
    monkeypatch.setattr(render, "MAP_BEV_SIDE", 64)                      # small pictures: the stand-in is numpy
    monkeypatch.setattr(render, "OBLIQUE_SIZE", (30, 40))
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    root, steps = _sequences(tmp_path), _hook_steps()
    # default: the PLYs of before and nothing else, no launch
    plain = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "plain"), str(root))
    assert plain.semantic_map["views"] == ()
    _epoch(plain, "val", steps)
    assert sorted(os.listdir(tmp_path / "plain")) == ["val_03_gt.ply", "val_03_pred.ply", "val_08_gt.ply", "val_08_pred.ply"]
    assert not draws.calls and all(p.endswith(".ply") for p in plain.semantic_map["paths"])
    # views: <step>_<sequence>_{pred,gt,err}_{view}.png of every sequence, before the maps are released
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps"), str(root), views=("bev", "oblique"))
    _epoch(stub, "val", steps)
    pngs = sorted(n for n in os.listdir(tmp_path / "maps") if n.endswith(".png"))
    assert pngs == sorted("val_%s_%s_%s.png" % (s, k, v) for s in ("03", "08") for k in ("pred", "gt", "err") for v in ("bev", "oblique"))
    assert sorted(n for n in os.listdir(tmp_path / "maps") if not n.endswith(".png")) == sorted(os.listdir(tmp_path / "plain"))
    assert sorted(os.path.basename(p) for p in stub.semantic_map["paths"] if p.endswith(".png")) == pngs
    assert stub.semantic_map["maps"] == {} and len(draws.calls) == 6 and sum(c["error"] for c in draws.calls) == 2
    assert all(np.array_equal(stub.logged_keys[key], plain.logged_keys[key]) for key in plain.logged_keys)     # the score is untouched
    bev = decode_png(str(tmp_path / "maps" / "val_08_pred_bev.png"))
    obl = decode_png(str(tmp_path / "maps" / "val_08_err_oblique.png"))
    assert obl.shape == render.OBLIQUE_SIZE + (3,) and bev.shape[2] == 3 and max(bev.shape[:2]) <= render.MAP_BEV_SIDE
    assert (bev != 255).any() and (obl != 255).any()                     # something was drawn
    with pytest.raises(ValueError, match="OCCDEPTH_MAP_VIEWS"):
        OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path), str(root), views=("camera",))


def test_map_views_are_switched_by_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def model():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg)
    for var in ("OCCDEPTH_MAP_VIEWS", "OCCDEPTH_MAP_MIN_OBS", "OCCDEPTH_FUSE", "OCCDEPTH_FUSE_POSES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OCCDEPTH_MAP_DIR", str(tmp_path / "maps"))
    monkeypatch.setenv("OCCDEPTH_MAP_POSES", str(tmp_path / "seq"))
    assert model().semantic_map["views"] == ()
    monkeypatch.setenv("OCCDEPTH_MAP_VIEWS", "bev,oblique")
    assert model().semantic_map["views"] == ("bev", "oblique")
    monkeypatch.setenv("OCCDEPTH_MAP_VIEWS", "bev,side")
    with pytest.raises(ValueError, match="OCCDEPTH_MAP_VIEWS"):
        model()


def test_map_sequence_tool_draws_and_is_unchanged_without_the_flags(monkeypatch, tmp_path, capsys):
    import pickle
    tool = _tool()
    KernelStandIn().install(monkeypatch)
    draws = MapRenderStandIn().install(monkeypatch)
    monkeypatch.setattr(render, "OBLIQUE_SIZE", (30, 40))                # small pictures: the stand-in is numpy
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    seq = tmp_path / "08"
    _write_sequence(seq, "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 0.4\n1 0 0 0.2 0 1 0 0 0 0 1 1.0\n")
    with open(seq / "calib.txt", "w") as f:                               # P2 with a baseline column, and Tr
        f.write("P0: 1 0 0 0 0 1 0 0 0 0 1 0\nP2: 30 0 15.5 1.2 0 30 9.5 0.3 0 0 1 0.002\nTr: 0 -1 0 0.5 0 0 -1 0.25 1 0 0 -0.125\n")
    pkl = tmp_path / "pkl"
    os.makedirs(pkl)
    for n, (lab, mask) in enumerate(frames_for(dims, C, 21, 3, masked=True)):
        with open(pkl / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": lab.astype(np.uint16), "target": np.roll(lab, 1, axis=0).astype(np.uint16),
                         "fov_mask_1": mask.reshape(-1)}, f)
    common = ["--poses", str(seq), "--pred", str(pkl), "--gt", str(pkl), "--dims", "16", "12", "8", "--origin"] + [str(o) for o in origin]

    def run(out, extra):
        tool.run(tool.parser().parse_args(common + ["--out", str(tmp_path / out / "08")] + extra), device=torch.device("cpu"))
        text = capsys.readouterr().out.replace(str(tmp_path / out), "<out>")
        return {n: open(tmp_path / out / n, "rb").read() for n in sorted(os.listdir(tmp_path / out))}, text
    before, text_before = run("a", [])
    assert sorted(before) == ["08_gt.ply", "08_pred.ply"] and not draws.calls and "pictures" not in text_before
    after, text_after = run("b", ["--views", "bev", "oblique", "--png-side", "64", "--camera-every", "2", "--camera-size", "20", "32",
                                  "--t-max", "4"])
    assert {n: after[n] for n in before} == before                       # byte-identical PLYs
    assert text_after.replace("<out>", "").startswith(text_before.split("map======")[0].replace("<out>", "")) and "map======" in text_after
    pngs = sorted(n for n in after if n.endswith(".png"))
    want = ["08_%s_%s.png" % (k, v) for k in ("pred", "gt", "err") for v in ("bev", "oblique")]
    want += ["08_%s_camera_%06d.png" % (k, f) for k in ("pred", "gt", "err") for f in (0, 2)]
    assert pngs == sorted(want) and "12 pictures" in text_after
    assert decode_png(str(tmp_path / "b" / "08_pred_camera_000002.png")).shape == (20, 32, 3)
    assert max(decode_png(str(tmp_path / "b" / "08_err_bev.png")).shape[:2]) <= 64
    assert [c["t_max"] for c in draws.calls if c["size"] == (20, 32)] == [4.0] * 6
    # calib.txt: cam_k = P2[:, :3], the extrinsic is Tr shifted by K^-1 P2[:, 3]
    k, E = tool.read_camera(str(seq))
    assert np.array_equal(k, [[30, 0, 15.5], [0, 30, 9.5], [0, 0, 1]])
    P2 = np.array([[30, 0, 15.5, 1.2], [0, 30, 9.5, 0.3], [0, 0, 1, 0.002]])
    Tr = np.array([[0, -1, 0, 0.5], [0, 0, -1, 0.25], [1, 0, 0, -0.125], [0, 0, 0, 1.0]])
    x = np.array([3.0, 0.7, -0.2, 1.0])
    assert np.allclose(k @ (E @ x)[:3], P2 @ (Tr @ x)) and np.array_equal(E[3], [0, 0, 0, 1])
    (seq / "calib.txt").write_text("Tr: 0 -1 0 0.5 0 0 -1 0.25 1 0 0 -0.125\n")
    with pytest.raises(KeyError, match="P2"):
        tool.read_camera(str(seq))


# ----------------------------------------------------------------------------------------------------- argument checks
def test_map_render_entry_point_rejects_bad_arguments(hip_lib):
    assert hip_lib.occd_map_render(None, None) == -1
    one = (ctypes.c_float * 32)()
    ptr = ctypes.addressof(one)

    def valid():
        a = hip.MapRenderArgs()
        a.labels = a.cells = a.views = a.palette = a.rgb = ptr
        a.gx = a.gy = a.gz = a.n_rows = a.n_views = a.H = a.W = 1
        a.n_palette, a.alpha, a.t_max = 4, 256, float("inf")
        return a
    edits = [("labels", None), ("cells", None), ("views", None), ("palette", None), ("rgb", None), ("gx", 0), ("gy", -1), ("gz", 0),
             ("gx", 65537), ("gz", 65537), ("n_rows", 0), ("n_views", 0), ("n_views", hip.RENDER_MAX_VIEWS + 1), ("H", 0), ("W", -1),
             ("n_palette", 0), ("n_palette", 65537), ("alpha", 257), ("alpha", -1), ("t_max", -1.0), ("t_max", float("nan")),
             ("flags", 2), ("flags", -1)]
    for field, value in edits:
        a = valid()
        setattr(a, field, value)
        assert hip_lib.occd_map_render(ctypes.byref(a), None) == -1, (field, value)
    a = valid()
    a.gx, a.gy, a.gz = 1024, 1024, 129                                   # more than 2^27 cells
    assert hip_lib.occd_map_render(ctypes.byref(a), None) == -1
    a = valid()
    a.target, a.n_palette = ptr, 3                                       # error mode needs the three error rows and a class
    assert hip_lib.occd_map_render(ctypes.byref(a), None) == -1
    a = valid()
    a.view_h[0] = 2                                                      # a view larger than the canvas
    assert hip_lib.occd_map_render(ctypes.byref(a), None) == -1
    assert ctypes.sizeof(hip.MapRenderArgs) == 10 * 8 + 11 * 4 + 2 * 8 * 4 + 4 and hip.ABI_VERSION == 22
    assert "occd_map_render" in hip.EXPORTS
    from occdepth_amd import build
    assert "map_render.hip" in build.SOURCES
