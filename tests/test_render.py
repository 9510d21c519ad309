"""CPU: the headless voxel renderer's host side (occdepth_amd/render.py) and the numpy restatement of its kernel.

`cast_ref` restates the traversal of csrc/render.hip and csrc/raycast.h (contract: include/occdepth_amd.h) step for step,
in the dtype it is given; `colour_ref` restates the integer colour rule.  tests/test_render_gpu.py compares the kernel with both.  Here the
restatement in float32 is compared with itself in float64, which pins how much float32 alone moves an image."""
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from occdepth_amd import render            # every test of this file needs it
from oracle import inputs

KITTI_VOXEL = 0.2


# ----------------------------------------------------------------------------------------------------- restatements
def rays(view, H, W, dtype):
    """The 18 floats of a view -> origin, dir (H, W, 3) in `dtype`, summed in the kernel's order."""
    g = np.asarray(view, dtype=np.float32).astype(dtype)
    fu = (np.arange(W, dtype=dtype) + dtype(0.5))[None, :, None]
    fv = (np.arange(H, dtype=dtype) + dtype(0.5))[:, None, None]
    return (g[0:3] + fu * g[3:6]) + fv * g[6:9], (g[9:12] + fu * g[12:15]) + fv * g[15:18]


def cast_ref(labels, origin, dirs, dtype, target=None):
    """First visible voxel along every ray -> hit (linear index or -1), face (3 on a miss), depth (inf on a miss)."""
    T = np.dtype(dtype).type
    X, Y, Z = labels.shape
    shape = origin.shape[:-1]
    o = np.ascontiguousarray(origin.reshape(-1, 3).astype(dtype))
    d = np.ascontiguousarray(dirs.reshape(-1, 3).astype(dtype))
    n = o.shape[0]
    dims = np.array([X, Y, Z], dtype=dtype)
    idims = np.array([X, Y, Z])
    flat = labels.reshape(-1).astype(np.int64)
    tflat = None if target is None else target.reshape(-1).astype(np.int64)
    inf = T(np.inf)
    with np.errstate(all="ignore"):
        alive = np.isfinite(o).all(1) & np.isfinite(d).all(1)
        nz = d != 0
        inv = np.where(nz, T(1) / np.where(nz, d, T(1)), T(0)).astype(dtype)
        tn, tf, axis = np.full(n, -inf, dtype), np.full(n, inf, dtype), np.full(n, 3)
        for a in range(3):                                       # slabs; a zero component is inside or outside
            ta, tc = (T(0) - o[:, a]) * inv[:, a], (dims[a] - o[:, a]) * inv[:, a]
            lo, hi = np.fmin(ta, tc), np.fmax(ta, tc)
            upd = nz[:, a] & (lo > tn)
            tn, axis = np.where(upd, lo, tn), np.where(upd, a, axis)
            tf = np.where(nz[:, a], np.fmin(tf, hi), tf)
            alive &= nz[:, a] | ((o[:, a] >= 0) & (o[:, a] < dims[a]))
        entered = tn > 0
        t = np.where(entered, tn, T(0)).astype(dtype)
        face = np.where(entered, axis, 3)
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
            lab = flat[vox]
            occ = (lab > 0) & (lab < 255)
            vis = occ if tflat is None else (tflat[vox] != 255) & (occ | (tflat[vox] != 0))
            hit[act[vis]] = vox[vis]
            alive[act[vis]] = False
            act = act[~vis]
            mm = m[act]
            ax = np.where((mm[:, 0] <= mm[:, 1]) & (mm[:, 0] <= mm[:, 2]), 0, np.where(mm[:, 1] <= mm[:, 2], 1, 2))
            mv = mm[np.arange(act.size), ax]
            go = mv < inf
            alive[act[~go]] = False
            act, ax, mv = act[go], ax[go], mv[go]
            idx[act, ax] += step[act, ax]
            ok = (idx[act, ax] >= 0) & (idx[act, ax] < idims[ax])
            alive[act[~ok]] = False
            act, ax, mv = act[ok], ax[ok], mv[ok]
            face[act], t[act] = ax, mv
            m[act, ax] = ((idx[act, ax] + (step[act, ax] > 0)).astype(dtype) - o[act, ax]) * inv[act, ax]
        assert not alive.any(), "the step bound was reached"
    miss = hit < 0
    return (hit.reshape(shape).astype(np.int32), np.where(miss, 3, face).reshape(shape).astype(np.uint8),
            np.where(miss, inf, t).reshape(shape).astype(dtype))


def colour_ref(labels, hit, face, pal, fov=None, target=None, background=None, alpha=256, bg=render.BACKGROUND):
    """The integer colour rule: hit / face (H, W) of one frame -> (H, W, 3) uint8."""
    pal = np.asarray(pal).astype(np.int64)
    P = pal.shape[0]
    h = np.maximum(hit, 0).astype(np.int64)
    lab = labels.reshape(-1).astype(np.int64)[h]
    if target is None:
        row = np.minimum(lab, P - 1)
    else:
        tg = target.reshape(-1).astype(np.int64)[h]
        occ = (lab > 0) & (lab < 255)
        err = P - 3
        row = np.where(~occ, err + render.ERR_FALSE_NEG,
                       np.where(tg == 0, err + render.ERR_FALSE_POS,
                                np.where(tg != lab, err + render.ERR_WRONG, np.minimum(lab, err - 1))))
    c = (pal[row] * np.asarray(render.SHADE, dtype=np.int64)[face.astype(np.int64)][..., None]) >> 8
    if fov is not None:
        c = np.where(fov.reshape(-1)[h][..., None] != 0, c, c // 3 * 2)
    if background is not None:
        back = background.astype(np.int64)
        c = (alpha * c + (256 - alpha) * back) >> 8
    else:
        back = np.broadcast_to(np.asarray(bg, dtype=np.int64), c.shape)
    return np.where((hit >= 0)[..., None], c, back).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ scenes
def make_scene(dims, seed):
    """Ground slab, a wall, random clutter, 2 % label 255, and the camera's cell carved out."""
    X, Y, Z = dims
    rng = np.random.RandomState(seed)
    vol = np.zeros(dims, dtype=np.uint8)
    vol[:, :, :2] = 9
    vol[(3 * X) // 4, :, :] = 13
    clutter = rng.rand(*dims) < 0.03
    vol[clutter] = rng.randint(1, 20, size=int(clutter.sum()))
    vol[rng.rand(*dims) < 0.02] = 255
    c = camera_cell(dims)
    vol[max(c[0] - 1, 0):c[0] + 2, max(c[1] - 1, 0):c[1] + 2, max(c[2] - 1, 0):c[2] + 2] = 0
    return vol


def kitti_calibration(W):
    """KITTI-like pinhole for a W-pixel-wide image (f = 707.09 W / 1220), the left camera's extrinsics, the origin."""
    k = inputs.KITTI_K.copy().astype(np.float64)
    k[:2] *= W / 1220.0
    return k, inputs.KITTI_TR.astype(np.float64)


def kitti_origin(dims):
    return (0.0, -0.5 * KITTI_VOXEL * dims[1], -2.0)


def camera_cell(dims):
    E = inputs.KITTI_TR.astype(np.float64)
    centre = -E[:3, :3].T @ E[:3, 3]
    g = (centre - np.array(kitti_origin(dims))) / KITTI_VOXEL
    return tuple(int(np.clip(np.floor(g[a]), 0, dims[a] - 1)) for a in range(3))


def scene_views(dims, cam_hw, bev_ppv=2, oblique_hw=None):
    """-> {name: (view (18,) float32 numpy, (H, W))} of the three kinds of view on a `dims` grid."""
    k, E = kitti_calibration(cam_hw[1])
    out = {"camera": (render.camera_view(torch.from_numpy(k), torch.from_numpy(E), kitti_origin(dims), KITTI_VOXEL).numpy(),
                      cam_hw),
           "bev": (render.bev_view(dims, bev_ppv, device="cpu").numpy(), render.bev_size(dims, bev_ppv))}
    if oblique_hw is not None:
        out["oblique"] = (render.oblique_view(dims, oblique_hw, -60.0, 35.0, device="cpu").numpy(), oblique_hw)
    return out


SCENES = {"24x20x12": ((24, 20, 12), (19, 61), (28, 45)), "64x64x16": ((64, 64, 16), (37, 122), (91, 122)),
          "128x128x32": ((128, 128, 32), (74, 244), (182, 244))}
MAX_DISAGREE = 1e-3


def disagreement(a, b):
    """Share of pixels whose (hit, face) differ, and the largest relative depth difference on the others."""
    same = (a[0] == b[0]) & (a[1] == b[1])
    both = same & (a[0] >= 0)
    da, db = a[2][both].astype(np.float64), b[2][both].astype(np.float64)
    rel = float(np.max(np.abs(da - db) / np.maximum(np.abs(db), 1.0))) if both.any() else 0.0
    return 1.0 - float(same.mean()), rel


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_restatement_against_float64(name):
    dims, cam_hw, obl_hw = SCENES[name]
    vol = make_scene(dims, seed=3)
    for vname, (view, (H, W)) in scene_views(dims, cam_hw, 2, obl_hw).items():
        r32 = cast_ref(vol, *rays(view, H, W, np.float32), np.float32)
        r64 = cast_ref(vol, *rays(view, H, W, np.float64), np.float64)
        share, rel = disagreement(r32, r64)
        hits = float((r64[0] >= 0).mean())
        print(f"{name} {vname} {W}x{H}: hits {hits:.3f} disagree {share:.2e} depth rel {rel:.2e}")
        assert hits > 0.2, (name, vname, hits)                  # the view does look at the scene
        assert share <= MAX_DISAGREE, (name, vname, share)
        assert rel < 1e-3, (name, vname, rel)
        if vname == "bev":
            assert share == 0.0


def test_traversal_edge_cases():
    vol = np.zeros((4, 3, 2), dtype=np.uint8)
    vol[1, 1, 1] = 5
    f = lambda o, d, dt=np.float32: [x.item() for x in cast_ref(vol, np.array([o], dtype=dt), np.array([d], dtype=dt), dt)]
    lin = (1 * 3 + 1) * 2 + 1
    assert f((1.5, 1.5, 1.5), (1, 0, 0)) == [lin, 3, 0.0]                    # inside an occupied voxel: t = 0, face 3
    assert f((1.5, 1.5, 1.5), (0, 0, 0)) == [lin, 3, 0.0]
    assert f((0.5, 1.5, 1.5), (0, 0, 0))[0] == -1                             # nothing to cross: terminates
    assert f((-2.0, 1.5, 1.5), (1, 0, 0)) == [lin, 0, 3.0]                    # enters through x, walks one voxel
    assert f((1.5, 1.5, 5.0), (0, 0, -1)) == [lin, 2, 3.0]                    # parallel to two axes
    assert f((1.5, 3.5, 5.0), (0, 0, -1))[0] == -1                            # parallel and outside
    assert f((-1e30, 1.5, 1.5), (0, 1, 0)) == [-1, 3, np.inf]
    assert f((np.nan, 1.5, 1.5), (1, 0, 0))[0] == -1 and f((0.5, 1.5, 1.5), (np.inf, 0, 0))[0] == -1
    assert f((-1.0, -1.0, 1.5), (1, 1, 0)) == [lin, 1, 2.0]                   # (0,0) -> (1,0) -> (1,1), both crossings at t = 2
    vol[1, 0, 1], vol[0, 1, 1] = 7, 8
    assert f((-1.0, -1.0, 1.5), (1, 1, 0)) == [(1 * 3 + 0) * 2 + 1, 0, 2.0]   # a tie between x and y: x is crossed first
    vol[:] = 0
    assert f((0.5, 0.5, 0.5), (1, 1, 1))[0] == -1                             # walks out of an empty grid


# ------------------------------------------------------------------------------------------------------------- views
def test_camera_view_hit_points_project_back_into_their_pixel():
    """The point origin + t dir of pixel (u, v), mapped to the world and projected with the float64 calibration the way
    the package projects voxels (x fx / z + cx, rounded), lands in pixel (u, v) at depth t."""
    dims, (H, W) = (64, 64, 16), (37, 122)
    k, E = kitti_calibration(W)
    org = np.array(kitti_origin(dims))
    view = render.camera_view(torch.from_numpy(k), torch.from_numpy(E), tuple(org), KITTI_VOXEL)
    assert view.dtype == torch.float32 and tuple(view.shape) == (18,)
    o, d = rays(view.numpy(), H, W, np.float64)
    for t in (2.5, 11.0):
        world = (o + d * t) * KITTI_VOXEL + org
        cam = world @ E[:3, :3].T + E[:3, 3]
        px, py = cam[..., 0] * k[0, 0] / cam[..., 2] + k[0, 2], cam[..., 1] * k[1, 1] / cam[..., 2] + k[1, 2]
        uu, vv = np.meshgrid(np.arange(W), np.arange(H))
        assert np.abs(px - uu).max() < 2e-3 and np.abs(py - vv).max() < 2e-3
        assert np.array_equal(np.rint(px), uu) and np.array_equal(np.rint(py), vv)
        assert np.abs(cam[..., 2] - t).max() < 1e-4
    # batched calibration and a per-frame origin tensor give one view per frame
    kb, Eb = torch.from_numpy(np.stack([k, k])), torch.from_numpy(np.stack([E, E]))
    vb = render.camera_view(kb, Eb, torch.from_numpy(np.stack([org, org + 1.0])), KITTI_VOXEL)
    assert tuple(vb.shape) == (2, 18) and torch.equal(vb[0], view) and not torch.equal(vb[1], view)


def test_camera_view_flip_mirrors_the_image():
    dims, (H, W) = (24, 20, 12), (19, 61)
    k, E = kitti_calibration(W)
    vol = make_scene(dims, seed=5)
    args = (torch.from_numpy(k), torch.from_numpy(E), kitti_origin(dims), KITTI_VOXEL)
    plain = cast_ref(vol, *rays(render.camera_view(*args).numpy(), H, W, np.float64), np.float64)
    flipped = cast_ref(vol, *rays(render.camera_view(*args, flip=True, width=W).numpy(), H, W, np.float64), np.float64)
    assert (plain[0] >= 0).mean() > 0.2
    share, rel = disagreement([x[:, ::-1] for x in flipped], plain)
    assert share <= MAX_DISAGREE and rel < 1e-5
    with pytest.raises(ValueError):
        render.camera_view(*args, flip=True)


def test_bev_view_is_first_occupied_from_the_top():
    dims = (24, 20, 12)
    vol = make_scene(dims, seed=7)
    vol[5, 6, :] = 0                                            # an empty column and a 255-only column: misses
    vol[7, 8, :] = 255
    H, W = render.bev_size(dims, 1)
    assert (H, W) == (24, 20)
    hit, face, depth = cast_ref(vol, *rays(render.bev_view(dims, 1, device="cpu").numpy(), H, W, np.float32), np.float32)
    occ = (vol > 0) & (vol < 255)
    top = np.where(occ.any(2), dims[2] - 1 - np.argmax(occ[:, :, ::-1], axis=2), -1)       # (X, Y) highest occupied z
    x, y = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), indexing="ij")
    want = np.where(top >= 0, (x * dims[1] + y) * dims[2] + top, -1)[::-1, ::-1]           # pixel (u, v) = (Y-1-y, X-1-x)
    assert np.array_equal(hit, want) and (hit[dims[0] - 1 - 5, dims[1] - 1 - 6] == -1) and (want >= 0).mean() > 0.9
    assert np.array_equal(face[hit >= 0], np.full((hit >= 0).sum(), 2))
    assert np.array_equal(depth[hit >= 0], (dims[2] - top[::-1, ::-1][hit >= 0]).astype(np.float32))


def test_oblique_view_sees_the_whole_volume():
    dims, (H, W) = (24, 20, 12), (45, 60)
    v = render.oblique_view(dims, (H, W), -60.0, 35.0, device="cpu").numpy()
    o, d = rays(v, H, W, np.float64)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0) and np.ptp(d.reshape(-1, 3), axis=0).max() == 0
    assert d[0, 0, 2] < 0 and np.allclose(v[3:6] @ v[9:12], 0, atol=1e-6) and np.allclose(v[6:9] @ v[9:12], 0, atol=1e-6)
    hit = cast_ref(np.ones(dims, dtype=np.uint8), o, d, np.float64)[0]
    assert (hit >= 0).mean() > 0.15 and (hit[0] == -1).all() and (hit[-1] == -1).all() and (hit[:, 0] == -1).all() \
        and (hit[:, -1] == -1).all()
    for corner in [(x, y, z) for x in (0, dims[0]) for y in (0, dims[1]) for z in (0, dims[2])]:     # all inside the image
        rel = np.array(corner, dtype=np.float64) - v[0:3]
        pu, pv = rel @ v[3:6] / (v[3:6] @ v[3:6]), rel @ v[6:9] / (v[6:9] @ v[6:9])
        assert 0 < pu < W and 0 < pv < H, corner
    top = np.array([dims[0] / 2, dims[1] / 2, dims[2]]) - v[0:3]
    bottom = np.array([dims[0] / 2, dims[1] / 2, 0.0]) - v[0:3]
    assert top @ v[6:9] < bottom @ v[6:9]                                                           # z is up in the image


# ------------------------------------------------------------------------------------------------------------ colour
def test_palettes():
    pk, pn, pg = render.palette("kitti"), render.palette("NYU"), render.palette(7)
    assert pk.dtype == torch.uint8 and tuple(pk.shape) == (23, 3) and tuple(pn.shape) == (15, 3) and tuple(pg.shape) == (10, 3)
    assert torch.equal(render.palette(20), pk) and torch.equal(render.palette(12), pn) and torch.equal(render.palette(7), pg)
    assert pk[1].tolist() == [100, 150, 245] and pk[9].tolist() == [255, 0, 255] and pk[0].tolist() == [0, 0, 0]
    for p in (pk, pn, pg):
        assert p[-3:].tolist() == [list(c) for c in render.ERROR_COLOURS]
        assert len({tuple(r) for r in p.tolist()}) == p.shape[0]            # all rows distinct
    with pytest.raises(ValueError):
        render.palette("nuscenes")


def test_colour_rule():
    pal = render.palette("kitti").numpy()
    labels = np.array([0, 1, 9, 19, 255, 300], dtype=np.uint16).reshape(6, 1, 1)
    hit = np.array([[1, 2, 3, -1, 5, 2, 2]], dtype=np.int32)
    face = np.array([[0, 1, 2, 3, 3, 3, 0]], dtype=np.uint8)
    got = colour_ref(labels, hit, face, pal)
    assert render.SHADE == (160, 208, 256, 256)
    assert got[0, 0].tolist() == [100 * 160 >> 8, 150 * 160 >> 8, 245 * 160 >> 8]
    assert got[0, 1].tolist() == [255 * 208 >> 8, 0, 255 * 208 >> 8]
    assert got[0, 2].tolist() == [255, 0, 0] and got[0, 3].tolist() == list(render.BACKGROUND)
    assert got[0, 4].tolist() == list(render.ERROR_COLOURS[2]) and got[0, 5].tolist() == [255, 0, 255]   # clamped row
    fov = np.array([1, 1, 0, 1, 1, 1], dtype=np.uint8)
    dim = colour_ref(labels, hit, face, pal, fov=fov)
    assert dim[0, 1].tolist() == [(255 * 208 >> 8) // 3 * 2, 0, (255 * 208 >> 8) // 3 * 2] and dim[0, 5].tolist() == [170, 0, 170]
    assert np.array_equal(dim[0, [0, 2, 3]], got[0, [0, 2, 3]])
    back = np.full((1, 7, 3), 50, dtype=np.uint8)
    back[0, 3] = (1, 2, 3)
    for alpha in (0, 128, 256):
        ov = colour_ref(labels, hit, face, pal, background=back, alpha=alpha)
        assert ov[0, 3].tolist() == [1, 2, 3]                                   # a miss is the background itself
        want = [(alpha * c + (256 - alpha) * 50) >> 8 for c in got[0, 0].tolist()]
        assert ov[0, 0].tolist() == want
    assert np.array_equal(colour_ref(labels, hit, face, pal, background=back, alpha=256)[0, :3], got[0, :3])
    assert np.array_equal(colour_ref(labels, hit, face, pal, background=back, alpha=0), back)


def test_error_mode_rule():
    pal = render.palette("kitti").numpy()
    pred = np.array([1, 1, 1, 0, 0, 1, 255], dtype=np.uint8).reshape(7, 1, 1)
    targ = np.array([1, 2, 0, 3, 0, 255, 4], dtype=np.uint8).reshape(7, 1, 1)
    # a ray down the x axis stops at the first voxel that is visible in error mode
    o, d = np.array([[-1.0, 0.5, 0.5]]), np.array([[1.0, 0.0, 0.0]])
    assert cast_ref(pred, o, d, np.float64, target=targ)[0].item() == 0
    for start, want in ((4, 6), (5, 6), (3, 3)):
        assert cast_ref(pred, o + [[start + 1.0, 0, 0]], d, np.float64, target=targ)[0].item() == want   # 4: both empty, 5: ignored
    hit = np.arange(7, dtype=np.int32)[None]
    got = colour_ref(pred, hit, np.full((1, 7), 2, dtype=np.uint8), pal, target=targ)
    e = [list(c) for c in render.ERROR_COLOURS]
    assert got[0, 0].tolist() == pal[1].tolist()                    # correct: the class colour
    assert got[0, 1].tolist() == e[render.ERR_WRONG] and got[0, 2].tolist() == e[render.ERR_FALSE_POS]
    assert got[0, 3].tolist() == e[render.ERR_FALSE_NEG] and got[0, 6].tolist() == e[render.ERR_FALSE_NEG]


# --------------------------------------------------------------------------------------------------------------- png
def decode_png(path):
    """A PNG as `write_png` writes it -> the array, checking signature, chunk order, CRCs and the row filters."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + W * ch)
    assert not rows[:, 0].any()                                     # filter 0 on every row
    return rows[:, 1:].reshape((H, W, 3) if ch == 3 else (H, W))


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 7, 3), (4, 61, 3), (3, 5)])
def test_write_png_round_trip(tmp_path, shape):
    img = np.random.RandomState(0).randint(0, 256, size=shape).astype(np.uint8)
    path = str(tmp_path / "a.png")
    assert render.write_png(path, img) == path
    assert np.array_equal(decode_png(path), img)
    render.write_png(path, torch.from_numpy(img).flip(0))           # a non-contiguous tensor
    assert np.array_equal(decode_png(path), img[::-1])
    with pytest.raises(ValueError):
        render.write_png(path, img.astype(np.float32))


# -------------------------------------------------------------------------------------------------------------- hook
def _stub(dataset="kitti"):
    return SimpleNamespace(dataset=dataset, full_scene_size=(64, 64, 16), render=None, RENDER_VOXEL_METRES={"kitti": 0.2, "NYU": 0.08},
                           _kitti_origin=lambda batch=None: (0.0, -6.4, -2.0))


def test_hook_is_off_by_default_and_validates(tmp_path, monkeypatch):
    from occdepth_amd.models.OccDepth import OccDepth
    from test_oracle_vs_golden import build_product
    for k in ("OCCDEPTH_RENDER_DIR", "OCCDEPTH_RENDER_EVERY", "OCCDEPTH_RENDER_MODE"):
        monkeypatch.delenv(k, raising=False)
    m = build_product("kitti_small")[0]
    assert m.render is None                                          # a model built as today has no render state
    stub = _stub()
    with pytest.raises(ValueError, match="view"):
        OccDepth.enable_render(stub, str(tmp_path), views=("camera", "side"))
    with pytest.raises(ValueError, match="mode"):
        OccDepth.enable_render(stub, str(tmp_path), mode="depth")
    with pytest.raises(ValueError):
        OccDepth.enable_render(stub, str(tmp_path), every=0)
    assert stub.render is None
    OccDepth.enable_render(stub, str(tmp_path), every=3, views=("bev", "oblique"), mode="error", max_frames=5)
    assert stub.render["every"] == 3 and stub.render["views"] == ("bev", "oblique") and stub.render["mode"] == "error"
    assert stub.render["written"] == 0 and not os.listdir(tmp_path)  # nothing happens until a step
    monkeypatch.setenv("OCCDEPTH_RENDER_DIR", str(tmp_path))
    monkeypatch.setenv("OCCDEPTH_RENDER_EVERY", "4")
    monkeypatch.setenv("OCCDEPTH_RENDER_MODE", "error")
    m = build_product("kitti_small")[0]
    assert m.render["out_dir"] == str(tmp_path) and m.render["every"] == 4 and m.render["mode"] == "error"


def test_camera_view_of_a_batch():
    from occdepth_amd.models.OccDepth import OccDepth
    k, E = kitti_calibration(122)
    batch = {"cam_k": [torch.from_numpy(np.stack([k, k]))] * 2, "T_velo_2_cam": [torch.from_numpy(np.stack([E, E + 1]).astype(np.float32))] * 2}
    stub = _stub()
    OccDepth.enable_render(stub, "unused", views=("camera", "bev", "oblique"))
    views, sizes = OccDepth._render_views(stub, batch, (64, 64, 16), (37, 122), "cpu")
    assert sizes == [(37, 122), (512, 512), render.OBLIQUE_SIZE] and [tuple(v.shape) for v in views] == [(2, 18), (18,), (18,)]
    want = render.camera_view(torch.from_numpy(k), torch.from_numpy(E.astype(np.float32)), (0.0, -6.4, -2.0), 0.2)
    assert torch.equal(views[0][1], want)                                  # the LEFT camera of each frame
    # another dataset: the calibration comes with the batch, cam_pose is inverted as a rigid transform
    nyu = _stub("NYU")
    nyu.full_scene_size = (60, 36, 60)
    OccDepth.enable_render(nyu, "unused", views=("camera",))
    with pytest.raises(NotImplementedError, match="cam_pose, vox_origin"):
        OccDepth._render_views(nyu, {"cam_k": batch["cam_k"]}, (60, 36, 60), (48, 64), "cpu")
    pose = np.linalg.inv(E)
    full = {"cam_k": [torch.from_numpy(k[None])], "cam_pose": [torch.from_numpy(pose)], "vox_origin": torch.tensor([[0.5, 0.25, -1.0]])}
    got = OccDepth._render_views(nyu, full, (60, 36, 60), (48, 64), "cpu")[0][0]
    ref = render.camera_view(torch.from_numpy(k), torch.from_numpy(E), (0.5, 0.25, -1.0), 0.08)
    assert tuple(got.shape) == (1, 18) and torch.allclose(got[0], ref, atol=1e-4, rtol=1e-5)
    OccDepth.enable_render(nyu, "unused", views=("bev", "oblique"))      # these need only the grid
    assert len(OccDepth._render_views(nyu, {}, (60, 36, 60), (48, 64), "cpu")[0]) == 2
    assert OccDepth._render_names(nyu, {"name": ["NYU0007_0000"]}, 0, 3) == ("", "NYU0007_0000")
    assert OccDepth._render_names(stub, {"sequence": ["08"], "frame_id": ["000125"]}, 0, 3) == ("08", "000125")


def test_render_logger_needs_add_image():
    from occdepth_amd.models.OccDepth import OccDepth
    exp = SimpleNamespace(add_image=lambda *a, **k: None)
    assert OccDepth._render_logger(SimpleNamespace(logger=SimpleNamespace(experiment=exp))) is exp
    assert OccDepth._render_logger(SimpleNamespace(logger=SimpleNamespace(experiment=object()))) is None
    assert OccDepth._render_logger(SimpleNamespace(logger=None)) is None and OccDepth._render_logger(SimpleNamespace()) is None


def test_render_labels_validates_before_any_launch():
    vol = torch.zeros(1, 4, 4, 2, dtype=torch.uint8)
    v = render.bev_view((4, 4, 2), 1, device="cpu")
    with pytest.raises(ValueError, match="mode"):
        render.render_labels(vol, v, (4, 4), mode="depth")
    with pytest.raises(ValueError, match="target"):
        render.render_labels(vol, v, (4, 4), mode="error")
    with pytest.raises(ValueError, match="views"):
        render.render_labels(vol, torch.zeros(17), (4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        render.render_labels(vol, v, (4, 4))                     # there is no CPU path


def test_entry_point_rejects_bad_arguments(hip_lib):
    import ctypes
    from occdepth_amd import hip
    assert hip_lib.occd_render_voxels(None, None) == -1
    one = (ctypes.c_float * 32)()
    ptr = ctypes.addressof(one)

    def valid():
        a = hip.RenderArgs()
        a.labels = a.views = a.palette = a.rgb = ptr
        a.batch = a.n_views = a.H = a.W = a.X = a.Y = a.Z = 1
        a.label_bytes, a.n_palette, a.alpha = 1, 4, 256
        return a
    edits = [("labels", None), ("views", None), ("palette", None), ("rgb", None), ("batch", 0), ("n_views", 0),
             ("n_views", hip.RENDER_MAX_VIEWS + 1), ("H", 0), ("W", -1), ("X", 0), ("Z", 0), ("label_bytes", 0),
             ("label_bytes", 3), ("label_bytes", 4), ("n_palette", 0), ("alpha", 257), ("alpha", -1)]
    for field, value in edits:
        a = valid()
        setattr(a, field, value)
        assert hip_lib.occd_render_voxels(ctypes.byref(a), None) == -1, (field, value)
    a = valid()
    a.target, a.target_bytes = ptr, 3
    assert hip_lib.occd_render_voxels(ctypes.byref(a), None) == -1
    a.target_bytes, a.n_palette = 1, 3                               # error mode needs the three error rows and a class
    assert hip_lib.occd_render_voxels(ctypes.byref(a), None) == -1
    a = valid()
    a.view_w[0] = 2                                                  # a view larger than the canvas
    assert hip_lib.occd_render_voxels(ctypes.byref(a), None) == -1
    a = valid()
    a.X = a.Y = 65536                                                # X Y Z beyond int32
    assert hip_lib.occd_render_voxels(ctypes.byref(a), None) == -1
    assert ctypes.sizeof(hip.RenderView) == 72 and hip.ABI_VERSION == 22
