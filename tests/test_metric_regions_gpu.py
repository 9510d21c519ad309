"""SSC confusion counts by region on the GPU (occd_ssc_confusion_regions) and the layers above it.  Every comparison is
exact integer equality against `np.bincount(C * t[m] + p[m])` over a boolean membership array; the FOV comes from
oracle.inputs.vox2pix.  Geometry: the kitti_small scene of tests/test_vox2pix_gpu.py at output scale (64 x 64 x 16 voxels
of 0.2 m, image 320 x 96), B = 2 with their own extrinsics, C = 20."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 20
DIMS = (64, 64, 16)
SCENE = (12.8, 12.8, 3.2)
VOX = 0.2
IMG = (320, 96)
ORIGIN = (0.0, -6.4, -2.0)
BOX_3M = (0, 16, 24, 40, 0, 16)
BOX_6M = (0, 32, 16, 48, 0, 16)


def _counts(t, p, m, n_classes=C):
    """(C, C) counts [target, prediction] over the membership array m (labelled voxels only)."""
    m = m & (t != 255) & (t < n_classes) & (p < n_classes)
    return np.bincount(n_classes * t[m].astype(np.int64) + p[m], minlength=n_classes * n_classes).reshape(n_classes, n_classes)


def _box_mask(box, dims=DIMS):
    m = np.zeros(dims, dtype=bool)
    m[box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
    return m


def _rows(logits, cs):
    """The 3-D stack's layout: a (B, C, X, Y, Z) view of (B, X, Y, Z, cs) channels-last rows."""
    B, c = logits.shape[:2]
    buf = torch.full((B,) + tuple(logits.shape[2:]) + (cs,), float("inf"), device=logits.device)     # pads would win an arg-max
    buf[..., :c] = logits.permute(0, 2, 3, 4, 1)
    return buf[..., :c].permute(0, 4, 1, 2, 3)


@pytest.fixture(scope="module")
def case():
    from oracle import inputs
    from test_vox2pix_gpu import _kitti_E
    g = np.random.default_rng(11)
    K = inputs.KITTI_K.copy()
    K[:2] *= 320 / 1220
    E = np.stack([_kitti_E(), _kitti_E()])                               # (B, V, 4, 4)
    E[1, :, :3, 3] += np.array([0.05, -0.03, 0.02])
    Kb = np.stack([np.stack([K, K])] * 2)
    Kb[1, :, 0, 0] *= 1.01
    fov = np.stack([np.stack([inputs.vox2pix(E[b, v], Kb[b, v], ORIGIN, VOX, IMG[0], IMG[1], SCENE, 0)[1][:, 0].reshape(DIMS)
                              for v in range(2)]) for b in range(2)])     # (B, V, X, Y, Z) bool
    logits = g.standard_normal((2, C) + DIMS).astype(np.float32)
    target = g.integers(0, C, size=(2,) + DIMS).astype(np.uint8)
    target[g.random((2,) + DIMS) < 0.1] = 255
    mask0 = g.random((2,) + DIMS) < 0.5
    pred = logits.argmax(1)
    out = dict(E=E, K=Kb, fov=fov, logits=logits, target=target, mask0=mask0, pred=pred,
               d_logits=torch.from_numpy(logits).to(DEV), d_target=torch.from_numpy(target).to(DEV),
               d_mask0=torch.from_numpy(mask0).to(DEV), d_E=torch.from_numpy(E).to(DEV), d_K=torch.from_numpy(Kb).to(DEV))
    for a in (E, Kb, fov, logits, target, mask0, pred):
        a.setflags(write=False)
    f0 = fov[:, 0]
    assert 0.5 < f0.mean() < 0.7 and 0.1 < f0[:, :16, 24:40].mean() < 0.3 and 0.3 < f0[:, :32, 16:48].mean() < 0.5
    return out


def _calib(case, views=(0,)):
    return (case["d_E"], case["d_K"], ORIGIN, VOX, IMG, views)


def _six_regions():
    from occdepth_amd import hip
    return [(None, 0), (None, hip.NEED_FOV), (BOX_3M, 0), (BOX_6M, 0), (BOX_3M, hip.NEED_FOV), (BOX_6M, hip.NEED_MASK0)]


def _six_expected(case, frames=slice(None)):
    t, p = case["target"][frames], case["pred"][frames]
    f = case["fov"][frames, 0]
    b3, b6 = _box_mask(BOX_3M)[None], _box_mask(BOX_6M)[None]
    one = np.ones_like(f)
    members = [one, f, one & b3, one & b6, f & b3, case["mask0"][frames] & b6]
    return np.stack([_counts(t, p, m) for m in members])


@pytest.mark.parametrize("layout", ["planes", "rows"])
def test_regions_and_layouts_gpu(hip_lib, case, layout):
    from occdepth_amd import hip
    logits = case["d_logits"] if layout == "planes" else _rows(case["d_logits"], 24)
    assert hip._logit_layout(logits)[1] == (DIMS[0] * DIMS[1] * DIMS[2] if layout == "planes" else 1)
    hist = torch.zeros(6, C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(hist, case["d_target"], _six_regions(), logits=logits, masks=[case["d_mask0"]],
                              fov=_calib(case))
    want = _six_expected(case)
    got = hist.cpu().numpy()
    for r in range(6):
        assert want[r].sum() > 0 and np.array_equal(got[r], want[r]), r
    assert want[1].sum() < want[0].sum() and want[4].sum() < want[2].sum()
    k7 = torch.zeros(C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion(k7, case["d_target"], logits=logits)
    assert torch.equal(k7, hist[0])


def test_fov_in_kernel_equals_explicit_mask_gpu(hip_lib, case):
    from occdepth_amd import hip
    _, table = hip.vox2pix(case["d_E"], case["d_K"], None, ORIGIN, VOX, DIMS, IMG)            # (B, V, N, 1) bool
    assert np.array_equal(table[..., 0].cpu().numpy().reshape(case["fov"].shape), case["fov"])
    regions = [(None, hip.NEED_FOV), (BOX_3M, hip.NEED_FOV), (BOX_6M, hip.NEED_FOV | hip.NEED_MASK0)]
    for views, explicit in (((0,), table[:, 0, :, 0]), ((0, 1), table[:, 0, :, 0] | table[:, 1, :, 0]), ((1,), table[:, 1, :, 0])):
        a = torch.zeros(3, C, C, dtype=torch.int64, device=DEV)
        b = torch.zeros_like(a)
        hip.ssc_confusion_regions(a, case["d_target"], regions, logits=case["d_logits"], masks=[case["d_mask0"]],
                                  fov=_calib(case, views))
        hip.ssc_confusion_regions(b, case["d_target"], regions, logits=case["d_logits"], masks=[case["d_mask0"]],
                                  fov=explicit.contiguous())
        assert torch.equal(a, b), views
        f = case["fov"][:, list(views)].any(1)
        assert np.array_equal(a[0].cpu().numpy(), _counts(case["target"], case["pred"], f)), views
    both = case["fov"].any(1)
    assert both.sum() > case["fov"][:, 0].sum()                                 # the second camera adds voxels


def test_per_frame_gpu(hip_lib, case):
    from occdepth_amd import hip
    args = dict(logits=_rows(case["d_logits"], 24), masks=[case["d_mask0"]], fov=_calib(case))
    shared = torch.zeros(6, C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(shared, case["d_target"], _six_regions(), **args)
    frames = torch.zeros(2, 6, C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(frames, case["d_target"], _six_regions(), per_frame=True, **args)
    for b in range(2):
        assert np.array_equal(frames[b].cpu().numpy(), _six_expected(case, slice(b, b + 1))), b
    assert not torch.equal(frames[0], frames[1])
    assert torch.equal(frames.sum(0), shared)


def test_labels_instead_of_logits_gpu(hip_lib, case):
    from occdepth_amd import hip
    labels = torch.from_numpy(case["pred"].astype(np.uint8)).to(DEV)
    hist = torch.zeros(6, C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(hist, case["d_target"], _six_regions(), labels=labels, masks=[case["d_mask0"]],
                              fov=_calib(case))
    assert np.array_equal(hist.cpu().numpy(), _six_expected(case))
    # predictions >= C are dropped in every region, like unlabelled targets
    labels2 = labels.clone()
    labels2[:, ::2] = 200
    two = torch.zeros(2, C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(two, case["d_target"], [(None, 0), (BOX_6M, 0)], labels=labels2)
    p2 = labels2.cpu().numpy()
    one = np.ones(case["target"].shape, dtype=bool)
    assert np.array_equal(two[0].cpu().numpy(), _counts(case["target"], p2, one))
    assert np.array_equal(two[1].cpu().numpy(), _counts(case["target"], p2, one & _box_mask(BOX_6M)[None]))


@pytest.mark.parametrize("layout", ["planes", "rows"])
def test_first_maximum_wins_gpu(hip_lib, case, layout):
    """Equal maxima at channels 3 and 7 count as 3 (np.argmax, K7)."""
    from occdepth_amd import hip
    x = case["d_logits"].clone()
    tie = torch.from_numpy(np.random.default_rng(5).random((2,) + DIMS) < 0.5).to(DEV)
    top = x.amax(1) + 1.0
    x[:, 3] = torch.where(tie, top, x[:, 3])
    x[:, 7] = torch.where(tie, top, x[:, 7])
    pred = x.cpu().numpy().argmax(1)
    assert (pred[tie.cpu().numpy()] == 3).all()
    hist = torch.zeros(2, C, C, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(hist, case["d_target"], [(None, 0), (BOX_3M, hip.NEED_FOV)],
                              logits=x if layout == "planes" else _rows(x, 24), fov=_calib(case))
    t = case["target"]
    assert np.array_equal(hist[0].cpu().numpy(), _counts(t, pred, np.ones(t.shape, dtype=bool)))
    assert np.array_equal(hist[1].cpu().numpy(), _counts(t, pred, case["fov"][:, 0] & _box_mask(BOX_3M)[None]))
    assert int(hist[0, :, 7].sum()) < int(hist[0, :, 3].sum())


@pytest.mark.parametrize("layout", ["planes", "rows", "rows_unaligned"])
def test_odd_grid_twelve_classes_gpu(hip_lib, layout):
    """C = 12 on 15 x 9 x 15 (the NYU output shape at a quarter): 2025 voxels per frame, so the last workgroup has a
    tail; a channels-last view whose base is not 16-byte aligned takes the binding's copy to planes."""
    from occdepth_amd import hip
    nc, dims = 12, (15, 9, 15)
    g = np.random.default_rng(2)
    logits = g.standard_normal((2, nc) + dims).astype(np.float32)
    target = g.integers(0, nc, size=(2,) + dims).astype(np.uint8)
    target[g.random((2,) + dims) < 0.1] = 255
    mask = g.random((2,) + dims) < 0.4
    box = (3, 15, 0, 7, 2, 15)
    x = torch.from_numpy(logits).to(DEV)
    if layout == "rows":
        x = _rows(x, 12)
        assert hip._logit_layout(x) == (2025 * 12, 1, 12)
    elif layout == "rows_unaligned":
        buf = torch.full((2,) + dims + (13,), float("inf"), device=DEV)
        buf[..., 1:] = x.permute(0, 2, 3, 4, 1)
        x = buf[..., 1:].permute(0, 4, 1, 2, 3)
        assert hip._logit_layout(x) is None
    hist = torch.zeros(3, nc, nc, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(hist, torch.from_numpy(target).to(DEV), [(None, 0), (box, 0), (box, hip.NEED_MASK0 << 2)],
                              logits=x, masks=[torch.from_numpy(mask).to(DEV)] * 3)
    pred = logits.argmax(1)
    bm = _box_mask(box, dims)[None]
    for r, m in enumerate((np.ones(target.shape, dtype=bool), np.ones(target.shape, dtype=bool) & bm, mask & bm)):
        assert np.array_equal(hist[r].cpu().numpy(), _counts(target, pred, m, nc)), r


def _reference_masked_stats(pred, true, nonempty, nonsurface, n_classes):
    """occdepth/loss/sscMetrics.py:70-109 restated: completion counts under labelled & nonempty & nonsurface (occupied =
    class > 0), per-class tp / fp / fn under labelled & nonempty."""
    lab = true != 255
    m_c, m_s = lab & nonempty & nonsurface, lab & nonempty
    bp, bt = pred[m_c] > 0, true[m_c] > 0
    tp, fp, fn = int((bt & bp).sum()), int((~bt & bp).sum()), int((bt & ~bp).sum())
    yp, yt = pred[m_s], true[m_s]
    tps = np.array([((yt == j) & (yp == j)).sum() for j in range(n_classes)], dtype=np.float64)
    fps = np.array([((yt != j) & (yp == j)).sum() for j in range(n_classes)], dtype=np.float64)
    fns = np.array([((yt == j) & (yp != j)).sum() for j in range(n_classes)], dtype=np.float64)
    precision, recall, iou = (tp / (tp + fp), tp / (tp + fn), tp / (tp + fp + fn)) if tp != 0 else (0, 0, 0)
    iou_ssc = tps / (tps + fps + fns + 1e-5)
    return {"precision": precision, "recall": recall, "iou": iou, "iou_ssc": iou_ssc, "iou_ssc_mean": np.mean(iou_ssc[1:])}


def test_add_batch_nonempty_nonsurface_gpu(hip_lib, case):
    """The reference's masked add_batch.  On the parent commit this raises NotImplementedError."""
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    g = np.random.default_rng(8)
    pred = case["pred"].astype(np.uint8)
    true = case["target"].copy()
    m1 = g.random(true.shape) < 0.7
    m2 = g.random(true.shape) < 0.6
    m = SSCMetrics(C, device=DEV)
    m.add_batch(pred, true, nonempty=m1, nonsurface=m2)
    got = m.get_stats()
    ref = _reference_masked_stats(pred, true, m1, m2, C)
    for k in ("precision", "recall", "iou", "iou_ssc_mean"):
        assert got[k] == ref[k], k
    assert np.array_equal(got["iou_ssc"], ref["iou_ssc"])
    # torch inputs on the device, uint8 masks, (B, N) masks: the same counts once more
    m.add_batch(torch.from_numpy(pred).to(DEV), case["d_target"], nonempty=torch.from_numpy(m1).to(DEV),
                nonsurface=m2.reshape(2, -1).astype(np.uint8))
    got2 = m.get_stats()
    assert got2["iou"] == ref["iou"] and int(m.masked_hist.sum()) == 2 * int((true != 255)[m1 & m2].sum() + (true != 255)[m1].sum())
    with pytest.raises(RuntimeError):
        m.add_batch(pred, true)


def test_accumulates_and_resets_in_place_gpu(hip_lib, case):
    from occdepth_amd import hip
    from occdepth_amd.loss.sscMetrics import Region, SSCMetrics
    hist = torch.full((6, C, C), 5, dtype=torch.int64, device=DEV)
    hip.ssc_confusion_regions(hist, case["d_target"], _six_regions(), logits=case["d_logits"], masks=[case["d_mask0"]],
                              fov=_calib(case))
    assert np.array_equal(hist.cpu().numpy(), _six_expected(case) + 5)
    regs = [Region("full"), Region("fov", fov=True), Region("3.2m", box=BOX_3M), Region("6.4m", box=BOX_6M),
            Region("fov_3.2m", box=BOX_3M, fov=True), Region("m0_6.4m", box=BOX_6M, masks=(0,))]
    m = SSCMetrics(C, regions=regs, per_frame=True)
    for _ in range(2):
        m.add_batch_logits(case["d_logits"], case["d_target"], fov=_calib(case), masks=[case["d_mask0"]])
    want = _six_expected(case)
    assert np.array_equal(m.region_hist.cpu().numpy(), 2 * want)
    from oracle.losses import metrics_from_confusion
    assert m.get_region_stats()["fov_3.2m"]["iou"] == metrics_from_confusion(2 * want[4])["iou"]
    fs = m.frame_stats()
    assert len(fs) == 4 and fs[3]["6.4m"]["iou"] == metrics_from_confusion(_six_expected(case, slice(1, 2))[3])["iou"]
    ptr = m.region_hist.data_ptr()
    m.reset()
    assert m.region_hist.data_ptr() == ptr and int(m.region_hist.abs().sum()) == 0 and m.frame_hists == []
    m.add_batch_logits(case["d_logits"], case["d_target"], fov=_calib(case), masks=[case["d_mask0"]])
    assert np.array_equal(m.region_hist.cpu().numpy(), want) and m.region_hist.data_ptr() == ptr


def test_captured_launch_replays_gpu(hip_lib, case):
    """The descriptors travel with the launch: three replays on refilled static inputs give three times one eager call."""
    from occdepth_amd import hip, train_graph
    logits = torch.zeros_like(case["d_logits"])
    target = torch.full_like(case["d_target"], 255)
    mask = torch.zeros_like(case["d_mask0"])
    E, K = torch.zeros_like(case["d_E"]), torch.zeros_like(case["d_K"])
    hist = torch.zeros(6, C, C, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    g = train_graph.new_graph()
    with torch.cuda.graph(g):
        hip.ssc_confusion_regions(hist, target, _six_regions(), logits=logits, masks=[mask], fov=(E, K, ORIGIN, VOX, IMG, (0,)))
    train_graph.seal_graph(g)
    hist.zero_()
    for src, dst in ((case["d_logits"], logits), (case["d_target"], target), (case["d_mask0"], mask), (case["d_E"], E),
                     (case["d_K"], K)):
        dst.copy_(src)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy(), 3 * _six_expected(case))


def test_model_eval_report_gpu(hip_lib, capsys):
    """enable_eval_report() on the kitti_small model, a batch WITHOUT fov tables: the ordinary metric and the reference's
    printed report are untouched, the `fov` region equals numpy counts over the oracle's mask at output scale."""
    from oracle import inputs
    from test_vox2pix_gpu import _kitti_E, _train_setup, _without
    m, full = _train_setup()
    m = m.eval()
    batch = _without(full)
    assert "fov_mask_1" not in batch
    with torch.no_grad():
        logits = m(batch)["ssc_logit"].detach().float().cpu().numpy()
        m.test_step(batch, 0)
        off_hist = m.test_metrics.hist.clone()
        assert m.report_metrics == {} and m.eval_report is None
        capsys.readouterr()
        m.test_epoch_end([])
        off_text = capsys.readouterr().out
        m.enable_eval_report()
        m.test_step(batch, 0)
        assert torch.equal(m.test_metrics.hist, off_hist)
        rep = m.report_metrics["test"]
        names = [r.name for r in rep.regions]
        assert names == ["full", "fov", "12.8m", "25.6m", "fov_12.8m", "fov_25.6m"]
        got = rep.region_hist.cpu().numpy()
        m.test_epoch_end([])
        on_text = capsys.readouterr().out
    n_cls = m.n_classes
    dims = tuple(int(s) for s in m.full_scene_size)
    assert logits.shape[2:] == dims
    target = full["target"].cpu().numpy()
    pred = logits.argmax(1)
    K = full["cam_k"][0][0].double().cpu().numpy()
    H, W = full["img"].shape[-2:]
    scene = tuple(d * 0.2 for d in dims)
    fov = np.stack([inputs.vox2pix(_kitti_E()[0], K, (0.0, -0.1 * dims[1], -2.0), 0.2, int(W), int(H), scene, 0)[1][:, 0]
                    .reshape(dims)] * target.shape[0])
    assert 0.02 < fov.mean() < 0.98
    assert np.array_equal(got[0], off_hist.cpu().numpy())
    assert np.array_equal(got[1], _counts(target, pred, fov, n_cls))
    assert np.array_equal(got[0], _counts(target, pred, np.ones_like(fov), n_cls))
    assert off_text.startswith("test======") and on_text.startswith(off_text)
    assert on_text[len(off_text):].startswith("test[full]======") and on_text.count("======") == 7
    assert rep.region_hist is not None and int(rep.region_hist.abs().sum()) == 0        # reset with the report
    # a batch that brings fov_mask_1 with the grid's size is believed: here the loader-shaped (V, N, 1) table carries
    # the RIGHT camera's mask in the left slot, which the calibration could not produce
    right = inputs.vox2pix(_kitti_E()[1], K, (0.0, -0.1 * dims[1], -2.0), 0.2, int(W), int(H), scene, 0)[1][:, :1]
    assert (right[:, 0].reshape(dims) != fov[0]).any()
    table = torch.from_numpy(np.stack([right, right])).to(DEV)
    with torch.no_grad():
        m.test_step(dict(batch, fov_mask_1=[table] * target.shape[0]), 0)
    got = m.report_metrics["test"].region_hist.cpu().numpy()
    assert np.array_equal(got[1], _counts(target, pred, np.stack([right[:, 0].reshape(dims)] * target.shape[0]), n_cls))
