"""GPU: occd_frame_visibility (K34) against `carve_ref`, the numpy float32 restatement of tests/test_visibility.py: every
byte of the marked volume is equal, and `hit` equals what occd_render_voxels reports for the same view.  The kernel
compiles with fp contraction off and the restatement rounds every product and sum once, so the comparison is exact.

Grids (40, 24, 20) and (16, 12, 8); a camera view of 47 x 157 pixels (neither a multiple of the 16 x 16 pixel workgroup;
on the small grid the camera stands outside the volume), a bird's-eye view (axis-parallel rays) and an oblique one; labels
of 1 and 2 bytes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from occdepth_amd import hip, render
from occdepth_amd import visibility as vis
from test_render import make_scene, rays, scene_views
from test_visibility import carve_ref

pytestmark = pytest.mark.gpu

GRIDS = [(40, 24, 20), (16, 12, 8)]
VIEWS = ["camera", "bev", "oblique"]


@functools.lru_cache(maxsize=None)
def scene(dims, label_bytes):
    vol = make_scene(dims, seed=11)
    if label_bytes == 2:
        vol = vol.astype(np.uint16)
        free = np.argwhere(vol == 0)
        for n, (x, y, z) in enumerate(free[:: max(1, len(free) // 40)]):    # labels past a byte: transparent, low byte or not
            vol[x, y, z] = (300, 261, 256, 65535)[n % 4]
    return vol


@functools.lru_cache(maxsize=None)
def reference(dims, label_bytes, name):
    view, (H, W) = scene_views(dims, (47, 157), 2, (45, 61))[name]
    visible, hit = carve_ref(scene(dims, label_bytes), *rays(view, H, W, np.float32), np.float32)
    return view, (H, W), visible, hit


def _labels(vol):
    return torch.from_numpy(vol if vol.dtype == np.uint8 else vol.view(np.int16)).cuda()


@pytest.mark.parametrize("name", VIEWS)
@pytest.mark.parametrize("label_bytes", [1, 2])
@pytest.mark.parametrize("dims", GRIDS, ids=["40x24x20", "16x12x8"])
def test_visibility_equals_the_restatement_and_hits_equal_the_renderer(dims, label_bytes, name):
    view, (H, W), want, want_hit = reference(dims, label_bytes, name)
    labels, dev_view = _labels(scene(dims, label_bytes)), torch.from_numpy(view).cuda()
    visible, hit = hip.frame_visibility(labels, dev_view, (H, W), return_hit=True)
    assert visible.dtype == torch.uint8 and tuple(visible.shape) == dims and hit.dtype == torch.int32 and tuple(hit.shape) == (H, W)
    assert np.array_equal(visible.cpu().numpy(), want)                       # every byte
    assert np.array_equal(hit.cpu().numpy(), want_hit)
    assert 0 < want.sum() < want.size and (want_hit >= 0).any()
    _, drawn, _, _ = hip.render_voxels(labels[None], dev_view[None, None], (H, W), render.palette("kitti").cuda(), aux=True)
    assert torch.equal(hit, drawn[0, 0])                                     # the renderer's first hit, pixel for pixel
    # without hit, through the module, and again over whatever the allocator hands back: the same bytes
    assert torch.equal(vis.visible_voxels(labels, dev_view, (H, W)), visible)
    assert torch.equal(hip.frame_visibility(labels, dev_view, (H, W)), visible)


def test_the_entry_point_zeroes_exactly_its_own_volume():
    """An output that starts 1, 2 or 15 bytes past a 16-byte boundary, in a buffer of 7s: the fill kernel's head and tail
    bytes, and nothing outside [0, X Y Z) is written."""
    dims = (16, 12, 8)
    view, (H, W), want, _ = reference(dims, 1, "camera")
    labels, dev_view = _labels(scene(dims, 1)), torch.from_numpy(view).cuda()
    S = dims[0] * dims[1] * dims[2]
    for shift, size in ((1, S), (2, S), (15, S), (0, S), (3, 9), (1, 40)):  # and volumes shorter than a piece or two
        buf = torch.full((S + 64,), 7, dtype=torch.uint8, device="cuda")
        a = hip.VisibilityArgs()
        a.labels, a.view, a.label_bytes = labels.data_ptr(), dev_view.data_ptr(), 1
        a.visible = buf.data_ptr() + 16 + shift
        assert buf.data_ptr() % 16 == 0
        a.H, a.W = H, W
        if size == S:
            a.X, a.Y, a.Z = dims
        else:
            a.X, a.Y, a.Z = size, 1, 1                                       # a row of `size` voxels cut from the volume's start
        assert hip.load().occd_frame_visibility(ctypes.byref(a), torch.cuda.current_stream().cuda_stream) == 0
        got = buf.cpu().numpy()
        lo = 16 + shift
        assert (got[:lo] == 7).all() and (got[lo + size:] == 7).all(), (shift, size)
        if size == S:
            assert np.array_equal(got[lo:lo + S], want.reshape(-1)), shift
        else:
            row = scene(dims, 1).reshape(-1)[:size].reshape(size, 1, 1)
            ref, _ = carve_ref(row, *rays(view, H, W, np.float32), np.float32)
            assert np.array_equal(got[lo:lo + size], ref.reshape(-1)), (shift, size)
