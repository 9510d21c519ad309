"""GPU: occd_map_render (K31) against occd_render_voxels on the densified window -- rgb, face, depth bits and the hit
mapped through the directory, equal on every pixel, no tolerance and no exclusions -- and against `map_cast_ref`, the
numpy restatement of tests/test_map_render.py; then the model hook writing real pictures.

Two maps: six frames voted into a SemanticMap pair on the GPU (grid (40, 24, 20), the sequence of tests/test_map.py: the
window has negative keys, over-selected bricks without a vote and a gap before the far frame), and the hand-placed
4 x 3 x 2 window of the CPU tests.  Five views in one launch with a size each -- (37, 61), (45, 28) and (19, 33) are no
multiple of the 8 x 8 tile -- camera inside the window, BEV, oblique, exact ties, two zero direction components."""
import functools
import os

import numpy as np
import pytest
import torch

from occdepth_amd import render
from occdepth_amd import semantic_map as sm
from test_map import GRIDS, V, _hook_steps, _hook_stub, _write_sequence, frames_for, sequence
from test_map_render import (BV, F, N_CLASSES, WINDOW_T_MAX, _rows_of, bits, dense_to_sparse_hit, densify, make_views,
                             window_case, window_refs, window_dense, with_t_max)
from test_render import colour_ref, decode_png

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("camera", "bev", "oblique", "tie", "zero")


def _voted(dims, C, seed, frames, masked):
    m = sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=8)
    poses = sequence(dims)
    for (lab, mask), f in zip(frames_for(dims, C, seed, len(frames), masked=masked), frames):
        m.integrate(torch.from_numpy(lab).to(DEV), poses[f], mask=None if mask is None else torch.from_numpy(mask).to(DEV))
    return m


def _placed(keys, rows, C=N_CLASSES):
    """A map whose bricks `keys` decide to the labels `rows` (n, 4096): one vote for the label, none where it is 255."""
    m = sm.SemanticMap(C, V, (0.0, 0.0, 0.0), (16, 16, 16), chunk_bricks=8)
    slots = m.slots(keys, create=True, device=DEV)
    votes = np.zeros((m.capacity, BV, m.pitch), dtype=np.int16)
    r, v = np.nonzero(rows != 255)
    votes[slots[r], v, rows[r, v]] = 1
    m.votes.copy_(torch.from_numpy(votes).view(m.votes.shape))
    return m


@functools.lru_cache(maxsize=None)
def volumes(name):
    """-> (pred map, gt map, MapVolume(pred, gt), views {name: (view, (H, W))}); built once, never changed."""
    if name == "voted":
        dims, C = (40, 24, 20), 12
        pred, gt = _voted(dims, C, 51, (0, 1, 2, 3, 4, 5), True), _voted(dims, C, 52, (0, 1, 2, 3, 4, 5), False)
        vol = sm.MapVolume(pred, gt)
        cam_at = np.array([-20.5, 0.5, 4.5]) - vol.origin_voxels          # 4 m behind the identity frame's sensor, 1 m up
        return pred, gt, vol, make_views(vol.dims, cam_at)
    case = window_case()
    pred, gt = _placed(case["keys"], case["labels"]), _placed(case["keys"], case["target"])
    return pred, gt, sm.MapVolume(pred, gt), case["views"]


def _launch_views(views):
    return [torch.from_numpy(views[n][0]) for n in NAMES], [views[n][1] for n in NAMES]


def _background(sizes, seed=5):
    H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(len(sizes), H, W, 3)).astype(np.uint8)).to(DEV)


@functools.lru_cache(maxsize=None)
def dense_result(name, mode, with_background):
    """occd_render_voxels on the densified window of the volume: per view (rgb, hit mapped to row * 4096 + local, face, depth)."""
    _, _, vol, views = volumes(name)
    rows_of = _rows_of(vol)
    dl = torch.from_numpy(densify(vol.labels.cpu().numpy(), rows_of)).to(DEV)
    dt = torch.from_numpy(densify(vol.target.cpu().numpy(), rows_of)).to(DEV) if mode == "error" else None
    assert tuple(dl.shape) == vol.dims
    vs, sizes = _launch_views(views)
    kw = {"background": _background(sizes)[None], "alpha": 100} if with_background else {}
    rgb, hit, face, depth = render.render_labels(dl[None], vs, sizes, target=dt, mode=mode, palette=vol.n_classes,
                                                 return_aux=True, **kw)
    return [(rgb[i][0].cpu().numpy(), dense_to_sparse_hit(hit[i][0].cpu().numpy(), rows_of), face[i][0].cpu().numpy(),
             depth[i][0].cpu().numpy()) for i in range(len(NAMES))]


def _sparse(vol, views, mode, with_background=False, **kw):
    vs, sizes = _launch_views(views)
    if with_background:
        kw.update(background=_background(sizes), alpha=100)
    out = render.render_map(vol, vs, sizes, mode=mode, palette=vol.n_classes, return_aux=True, **kw)
    return [tuple(out[j][i].cpu().numpy() for j in range(4)) for i in range(len(NAMES))]


def _assert_same(got, want, what):
    for i, name in enumerate(NAMES):
        assert got[i][0].shape == want[i][0].shape, (what, name)
        for j, part in enumerate(("rgb", "hit", "face")):
            assert np.array_equal(got[i][j], want[i][j]), (what, name, part, int((got[i][j] != want[i][j]).sum()))
        assert np.array_equal(bits(got[i][3]), bits(want[i][3])), (what, name, "depth")


@pytest.mark.parametrize("with_background", [False, True], ids=["plain", "background"])
@pytest.mark.parametrize("mode", ["class", "error"])
@pytest.mark.parametrize("name", ["voted", "placed"])
def test_sparse_walk_equals_the_dense_renderer_on_every_pixel(hip_lib, name, mode, with_background):
    pred, gt, vol, views = volumes(name)
    if name == "voted":
        keys = vol.keys
        cells = vol.cells.cpu().numpy()
        assert (keys.min(0) < 0).any() and (cells < 0).sum() > 0 and (~vol.drawable.cpu().numpy()).any()
    want = dense_result(name, mode, with_background)
    got = _sparse(vol, views, mode, with_background)
    assert got[0][1].dtype == np.int64 and got[0][2].dtype == np.uint8 and got[0][3].dtype == F
    _assert_same(got, want, (name, mode))
    for i, n in enumerate(NAMES):
        hits = got[i][1] >= 0
        assert hits.any() and ((~hits).any() or name == "voted"), n     # the voted map is a wall of labels to its camera
        assert np.isposinf(got[i][3][~hits]).all() and (got[i][2][~hits] == 3).all()


@pytest.mark.parametrize("mode", ["class", "error"])
@pytest.mark.parametrize("name", ["voted", "placed"])
def test_skip_off_and_kept_empty_bricks_give_the_same_pictures(hip_lib, name, mode):
    pred, gt, vol, views = volumes(name)
    first = _sparse(vol, views, mode)
    _assert_same(_sparse(vol, views, mode, skip=False), first, "skip=False")
    full = sm.MapVolume(pred, gt, drop_empty=False)
    assert (full.cells >= 0).sum() > (vol.cells >= 0).sum() and torch.equal(full.labels, vol.labels)
    _assert_same(_sparse(full, views, mode), first, "drop_empty=False")
    _assert_same(_sparse(vol, views, mode, skip=False, t_max=WINDOW_T_MAX), _sparse(vol, views, mode, t_max=WINDOW_T_MAX), "t_max, skip=False")


@pytest.mark.parametrize("mode", ["class", "error"])
@pytest.mark.parametrize("name", ["voted", "placed"])
def test_finite_t_max_turns_deeper_hits_into_misses(hip_lib, name, mode):
    _, _, vol, views = volumes(name)
    dense = dense_result(name, mode, False)
    got = _sparse(vol, views, mode, t_max=WINDOW_T_MAX)
    background = np.array(render.BACKGROUND, dtype=np.uint8)
    cut = 0
    for i, n in enumerate(NAMES):
        hit, face, depth = with_t_max(dense[i][1:], WINDOW_T_MAX)
        far = (dense[i][1] >= 0) & (hit < 0)
        cut += int(far.sum())
        assert np.array_equal(got[i][1], hit) and np.array_equal(got[i][2], face) and np.array_equal(bits(got[i][3]), bits(depth)), n
        assert np.array_equal(got[i][0], np.where(far[..., None], background, dense[i][0])), n
    assert cut > 0


@pytest.mark.parametrize("t_max", [np.inf, WINDOW_T_MAX], ids=["inf", "finite"])
@pytest.mark.parametrize("mode", ["class", "error"])
def test_kernel_equals_the_numpy_restatement(hip_lib, mode, t_max):
    """Ties the kernel to the numpy statement of the two-level walk itself, not only to K27 -- and, end to end, the
    error-mode picture of MapVolume(pred, gt) to `colour_ref` on the hand-placed labels."""
    case = window_case()
    _, _, vol, views = volumes("placed")
    assert np.array_equal(vol.labels.cpu().numpy(), case["labels"]) and np.array_equal(vol.target.cpu().numpy(), case["target"])
    assert np.array_equal(vol.cells.cpu().numpy(), case["cells"]) and np.array_equal(vol.key_min, case["keys"].min(0))
    refs = window_refs(mode, t_max)
    got = _sparse(vol, views, mode, t_max=None if t_max == np.inf else t_max)
    pal = render.palette(N_CLASSES).numpy()
    for i, n in enumerate(NAMES):
        hit, face, depth, _ = refs[n]
        assert np.array_equal(got[i][1], hit) and np.array_equal(got[i][2], face) and np.array_equal(bits(got[i][3]), bits(depth)), n
        want = colour_ref(case["labels"], hit, face, pal, target=case["target"] if mode == "error" else None)
        assert np.array_equal(got[i][0], want), n
    if t_max == np.inf:                                                  # and the restatement is the dense walk (CPU test)
        dense = window_dense(mode)
        assert all(np.array_equal(got[i][1], dense[n][0]) for i, n in enumerate(NAMES))


def test_uniform_size_and_single_view(hip_lib):
    _, _, vol, views = volumes("placed")
    view = torch.from_numpy(views["camera"][0])
    rgb = render.render_map(vol, view, (37, 61))
    assert tuple(rgb.shape) == (1, 37, 61, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda
    both = render.render_map(vol, torch.stack([view, view]), (40, 64), mode="error")
    assert tuple(both.shape) == (2, 40, 64, 3) and torch.equal(both[0], both[1])
    assert torch.equal(render.render_map(vol, view, (40, 64), mode="error")[0], both[0])
    assert torch.equal(render.render_map(vol, view, (40, 64))[0, :37, :61], rgb[0])


def test_model_hook_writes_the_pictures_of_real_maps(hip_lib, tmp_path):
    from occdepth_amd import fuse, hip
    from occdepth_amd.models.OccDepth import OccDepth
    from test_map import HOOK_C, HOOK_DIMS, HOOK_ORIGIN
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps"), str(root), views=("bev", "oblique"))
    steps = [({k: v for k, v in batch.items() if k != "fov_mask_1"}, logits.to(DEV), target.to(DEV)) for batch, logits, target in _hook_steps()]
    for batch, logits, target in steps:
        OccDepth._map_step(stub, "val", batch, logits, target)
    assert OccDepth._map_epoch_end(stub, "val") is not None and stub.semantic_map["maps"] == {}
    names = sorted(os.listdir(tmp_path / "maps"))
    assert sorted(n for n in names if n.endswith(".png")) == sorted(
        "val_%s_%s_%s.png" % (s, k, v) for s in ("03", "08") for k in ("pred", "gt", "err") for v in ("bev", "oblique"))
    assert sorted(os.path.basename(p) for p in stub.semantic_map["paths"]) == names
    # the same maps, voted here, drawn by the public function: the files hold those pictures
    vs = 0.2
    for seq in ("03", "08"):
        poses = fuse.read_kitti_poses(str(root / seq))
        pair = [sm.SemanticMap(HOOK_C, vs, HOOK_ORIGIN, HOOK_DIMS) for _ in range(2)]
        for batch, logits, target in steps:
            for i, s in enumerate(batch["sequence"]):
                if s == seq:
                    P = poses[int(batch["frame_id"][i])]
                    pair[0].integrate(hip.argmax_labels_u16(logits[i:i + 1])[0], P)
                    pair[1].integrate(target[i], P)
        vol = sm.MapVolume(pair[0], pair[1])
        views, sizes = render.map_standard_views(("bev", "oblique"), vol)
        assert sizes[1] == render.OBLIQUE_SIZE and max(sizes[0]) <= render.MAP_BEV_SIDE
        for kind, v, mode in (("pred", vol, "class"), ("gt", vol.target_volume(), "class"), ("err", vol, "error")):
            want = render.render_map(v, views, sizes, mode=mode)
            for name, img in zip(("bev", "oblique"), want):
                got = decode_png(str(tmp_path / "maps" / ("val_%s_%s_%s.png" % (seq, kind, name))))
                assert np.array_equal(got, img.cpu().numpy()), (seq, kind, name)
                assert (got != 255).any()
