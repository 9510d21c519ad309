"""GPU: occd_ray_metric (K35) against `ray_metric_ref`, the numpy restatement of tests/test_ray_metric.py (two independent
float32 `cast_ref` walks per origin, then counting): every counter is equal.  The kernel compiles with fp contraction off
and the restatement rounds every product and sum once, so the comparison is exact.

Scenes: make_scene (24, 20, 12), (64, 64, 16) and (128, 128, 32) as targets, the target rolled one voxel along x with
255 -> 0 and 20 % of the occupied labels redrawn as predictions, 16 beams x 90 azimuths (1440 rays: 5 workgroups and a
half wave) from the KITTI sensor origin.  On the restatement alone (tests/test_ray_metric.py pins them): valid rays 1015 /
1324 / 1421 in pass mode, 915 / 929 / 722 in drop mode with 214 / 469 / 711 rays in `unknown`."""
import numpy as np
import pytest
import torch

from occdepth_amd import hip, render, train_graph
from occdepth_amd import ray_metric as rm
from test_ray_metric import (EXPECT, SCENES, THR_M, RayStandIn, grid_thresholds, guard, make_prediction, ray_metric_ref, scene,
                             split)
from test_render import KITTI_VOXEL, make_scene, rays, scene_views

pytestmark = pytest.mark.gpu

C = 20
MODES = {"drop": hip.RAY_UNKNOWN_DROP, "pass": hip.RAY_UNKNOWN_PASS}


def _dev(vol):
    vol = np.ascontiguousarray(vol)
    return torch.from_numpy(vol.view(np.int16) if vol.dtype == np.uint16 else vol.copy()).cuda()


def run(pred, target, origins, dirs, thresholds, n_classes=C, mode="drop", counts=None):
    """pred, target (B, X, Y, Z) numpy; origins (B, K, 3); dirs (N, 3); thresholds in grid units -> the counters (numpy)."""
    if counts is None:
        counts = torch.zeros(hip.ray_metric_size(n_classes, len(thresholds)), dtype=torch.int64, device="cuda")
    out = hip.ray_metric(_dev(pred), _dev(target), torch.from_numpy(np.array(origins, dtype=np.float32)).cuda(),
                         torch.from_numpy(np.array(dirs, dtype=np.float32)).cuda(), counts, [float(t) for t in thresholds],
                         n_classes, MODES[mode])
    assert out is counts
    return counts.cpu().numpy()


@pytest.mark.parametrize("mode", ["drop", "pass"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_counter_equals_the_restatement(name, mode):
    target, pred, origin, dirs, ref = scene(name)
    got = run(pred[None], target[None], origin[None, None], dirs, grid_thresholds(THR_M), mode=mode)
    c = split(got, C, 3)
    print(name, mode, "valid", c.valid, "unknown", c.unknown, "pred_miss", c.pred_miss, "tp", c.tp.sum(1).tolist(), "tp_geo",
          c.tp_geo.tolist())
    guard(c, mode)                                                           # an all-zero kernel cannot pass
    assert (c.valid, c.unknown) == EXPECT[name][mode]
    assert np.array_equal(got, ref[mode])


def _wide(vol, seed):
    """2-byte labels: the volume with labels past a byte in free voxels (transparent, whatever their low byte)."""
    out = vol.astype(np.uint16)
    free = np.argwhere(out == 0)
    for n, (x, y, z) in enumerate(free[seed:: max(1, len(free) // 60)]):
        out[x, y, z] = (300, 261, 256, 65535, 511)[n % 5]
    return out


@pytest.mark.parametrize("pred_bytes,target_bytes", [(1, 2), (2, 1), (2, 2)])
def test_label_widths(pred_bytes, target_bytes):
    target, pred, origin, dirs, ref = scene("24x20x12")
    p = _wide(pred, 1) if pred_bytes == 2 else pred
    t = _wide(target, 2) if target_bytes == 2 else target
    for mode in ("drop", "pass"):
        got = run(p[None], t[None], origin[None, None], dirs, grid_thresholds(THR_M), mode=mode)
        assert np.array_equal(got, ref[mode])                                # the wide labels are seen through: nothing moves
        assert np.array_equal(got, ray_metric_ref(p[None], t[None], origin[None, None], dirs, grid_thresholds(THR_M), C, mode))


def test_batch_origins_ragged_rays_thresholds_and_accumulation():
    """B = 2 different volumes, K = 3 origins (inside the grid, outside it, inside an occupied voxel), N = 1433 rays (no
    multiple of 64), 1 and 4 thresholds, n_classes below the largest label, two calls into the same counters."""
    dims = (24, 20, 12)
    ta, pa, origin, dirs, _ = scene("24x20x12")
    tb = make_scene(dims, 11)
    pb = make_prediction(tb, 11)
    preds, targets = np.stack([pa, pb]), np.stack([ta, tb])
    occupied = np.argwhere((ta > 0) & (ta < 255) & (tb == 0))[40]            # occupied in frame 0's target, free in frame 1's
    inside = origin + np.float32(0.25)
    origins = np.stack([inside, np.array([-6.5, 31.0, 17.25], np.float32), occupied.astype(np.float32) + np.float32(0.5)])
    origins = np.stack([origins, origins[::-1]])                             # (2, 3, 3): the frames take them in another order
    d = dirs[:1433]
    for thr_m, n_classes in (((2.0,), C), ((0.5, 1.0, 2.0, 4.0), C), (THR_M, 12)):
        thr = grid_thresholds(thr_m)
        for mode in ("drop", "pass"):
            want = ray_metric_ref(preds, targets, origins, d, thr, n_classes, mode)
            got = run(preds, targets, origins, d, thr, n_classes, mode)
            c = split(got, n_classes, len(thr))
            assert c.rays == 2 * 3 * 1433 and c.valid > 0.3 * c.rays and c.pred_miss > 0
            assert np.array_equal(got, want), (thr_m, n_classes, mode)
    # the counters are added to, never zeroed
    counts = torch.zeros(hip.ray_metric_size(C, 3), dtype=torch.int64, device="cuda")
    thr = grid_thresholds(THR_M)
    run(preds, targets, origins, d, thr, counts=counts)
    twice = run(preds[::-1], targets[::-1], origins, d, thr, counts=counts)
    want = ray_metric_ref(preds, targets, origins, d, thr, C) + ray_metric_ref(preds[::-1], targets[::-1], origins, d, thr, C)
    assert np.array_equal(twice, want)
    # the origin inside an occupied voxel hits it at depth 0, whatever the direction
    alone = split(run(ta[None], ta[None], origins[:1, 2:], d, thr, mode="pass"), C, 3)
    assert alone.valid == 1433 and alone.gt[ta[tuple(occupied)]] == 1433 and alone.tp[0].sum() == 1433


def test_tiled_and_beam_major_rays_give_equal_counters():
    target, pred, origin, dirs, ref = scene("64x64x16")
    plain = rm.lidar_directions(beams=16, azimuth_step_deg=2.0, tile=None).numpy()
    assert not np.array_equal(plain, dirs)
    for mode in ("drop", "pass"):
        assert np.array_equal(run(pred[None], target[None], origin[None, None], plain, grid_thresholds(THR_M), mode=mode), ref[mode])


def test_non_finite_rays_count_as_rays_only():
    target, pred, origin, dirs, _ = scene("24x20x12")
    bad = dirs[:70].copy()
    bad[3, 0], bad[40, 2], bad[69, 1] = np.nan, np.inf, -np.inf
    thr = grid_thresholds(THR_M)
    got = run(pred[None], target[None], origin[None, None], bad, thr)
    assert np.array_equal(got, ray_metric_ref(pred[None], target[None], origin[None, None], bad, thr, C)) and got[0] == 70
    nowhere = run(pred[None], target[None], np.full((1, 1, 3), np.nan, np.float32), dirs, thr)
    assert nowhere[0] == 1440 and not nowhere[1:].any()


def test_ray_metrics_on_the_gpu_equals_the_stand_in_path(monkeypatch):
    target, pred, origin, dirs, ref = scene("24x20x12")
    tb = make_scene((24, 20, 12), 11)
    pb = make_prediction(tb, 11)
    preds, targets = np.stack([pred, pb]), np.stack([target, tb])
    origins = np.stack([origin, origin + np.float32(1.5)])

    def feed(device):
        m = rm.RayMetrics(C, KITTI_VOXEL, dirs)
        m.add_batch(torch.from_numpy(pred[None].copy()).to(device), torch.from_numpy(target[None].copy()).to(device),
                    torch.from_numpy(origin.copy()))
        m.add_batch(torch.from_numpy(preds.astype(np.int64)).to(device), torch.from_numpy(targets.astype(np.int32)).to(device),
                    torch.from_numpy(origins))
        return m

    on_gpu = feed("cuda")
    assert on_gpu.counts().is_cuda and np.array_equal(on_gpu.counts()[:ref["drop"].size].cpu().numpy() - ref["drop"],
                                                      ray_metric_ref(preds, targets, np.broadcast_to(origins, (2, 2, 3)), dirs,
                                                                     grid_thresholds(THR_M), C))
    RayStandIn().install(monkeypatch)
    stand_in = feed("cpu")
    assert torch.equal(on_gpu.counts().cpu(), stand_in.counts())
    a, b = on_gpu.get_stats(), stand_in.get_stats()
    assert a["RayIoU"] == b["RayIoU"] and 0.0 < a["RayIoU"] < 1.0 and np.array_equal(a["ray_iou"], b["ray_iou"])
    assert np.array_equal(a["ray_iou_geo"], b["ray_iou_geo"])
    merged = rm.RayMetrics(C, KITTI_VOXEL, dirs).merge_(on_gpu).merge_(stand_in.counts())
    assert torch.equal(merged.counts().cpu(), 2 * stand_in.counts())


def test_prediction_hits_agree_with_the_renderer(name="camera"):
    """On the rays of an affine pinhole view, with a target every ray that enters the grid hits at once (all voxels
    occupied): valid, pred_miss and pred[] are what occd_render_voxels' hit buffer gives for the same rays."""
    dims = (64, 64, 16)
    pred = make_scene(dims, 3)
    view, (H, W) = scene_views(dims, (37, 122), 2, (45, 61))[name]
    assert not view[3:9].any()                                               # a pinhole: one origin for every pixel
    _, d = rays(view, H, W, np.float32)
    full = np.ones(dims, dtype=np.uint8)
    palette = render.palette("kitti").cuda()
    dev_view = torch.from_numpy(view).cuda()[None, None]
    hit_p = hip.render_voxels(_dev(pred[None]), dev_view, (H, W), palette, aux=True)[1].cpu().numpy().reshape(-1)
    hit_t = hip.render_voxels(_dev(full[None]), dev_view, (H, W), palette, aux=True)[1].cpu().numpy().reshape(-1)
    entered = hit_t >= 0
    assert 0.2 < (hit_p >= 0).mean() < 1.0 and entered.any() and not (hit_p >= 0)[~entered].any()
    got = split(run(pred[None], full[None], view[None, None, 0:3], d.reshape(-1, 3), grid_thresholds(THR_M), mode="pass"), C, 3)
    assert got.rays == H * W and got.valid == int(entered.sum()) and got.gt[1] == got.valid
    assert got.pred_miss == int((entered & (hit_p < 0)).sum())
    assert np.array_equal(got.pred, np.bincount(pred.reshape(-1)[hit_p[hit_p >= 0]], minlength=C)[:C])


def test_capture_and_replay():
    """Captured on one stream (no parallel branches): two replays add twice what one eager call adds."""
    target, pred, origin, dirs, ref = scene("24x20x12")
    m = rm.RayMetrics(C, KITTI_VOXEL, dirs)
    p, t = torch.from_numpy(pred[None].copy()).cuda(), torch.from_numpy(target[None].copy()).cuda()
    o = torch.from_numpy(origin.copy()).cuda().reshape(1, 1, 3)
    m.add_batch(p, t, o)                                                     # eager: allocates the counters, moves the rays
    eager = m.counts().clone()
    assert np.array_equal(eager.cpu().numpy(), ref["drop"])
    m.reset()
    torch.cuda.synchronize()
    g = train_graph.new_graph()
    with torch.cuda.graph(g):
        m.add_batch(p, t, o)
    train_graph.seal_graph(g)
    torch.cuda.synchronize()
    assert not m.counts().any()                                              # capturing ran nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.counts(), 2 * eager)
