"""CPU: the host side of the SSC metrics by region -- metre -> index boxes, statistics per region, the nonempty /
nonsurface form of `add_batch` (orchestration only, through a torch stand-in of the kernel), the argument checks of
occd_ssc_confusion_regions before any launch, and the unchanged default path."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd.loss.sscMetrics import Region, SSCMetrics, metric_box

KITTI_ORIGIN = (0.0, -25.6, -2.0)
KITTI_GRID = (256, 256, 32)


# ------------------------------------------------------------------------------------------------------------ boxes
def test_kitti_ranges_in_voxels():
    assert metric_box((0.0, 12.8, -6.4, 6.4), KITTI_ORIGIN, 0.2, KITTI_GRID) == (0, 64, 96, 160, 0, 32)
    assert metric_box((0.0, 25.6, -12.8, 12.8), KITTI_ORIGIN, 0.2, KITTI_GRID) == (0, 128, 64, 192, 0, 32)
    assert metric_box((0.0, 51.2, -25.6, 25.6), KITTI_ORIGIN, 0.2, KITTI_GRID) == (0, 256, 0, 256, 0, 32)


def test_metric_box_rounds_to_the_nearest_edge_and_clips():
    # 0.29 m -> edge 1 (0.2 m), 0.31 m -> edge 2 (0.4 m); z given explicitly
    assert metric_box((0.29, 0.71, -25.6, -25.29, -2.0, -1.0), KITTI_ORIGIN, 0.2, KITTI_GRID) == (1, 4, 0, 2, 0, 5)
    # beyond the grid on every side: clipped
    assert metric_box((-5.0, 80.0, -40.0, 40.0, -9.0, 9.0), KITTI_ORIGIN, 0.2, KITTI_GRID) == (0, 256, 0, 256, 0, 32)
    # the reduced test scene: 12.8 m wide, origin (0, -6.4, -2)
    assert metric_box((0.0, 25.6, -12.8, 12.8), (0.0, -6.4, -2.0), 0.2, (64, 64, 16)) == (0, 64, 0, 64, 0, 16)


@pytest.mark.parametrize("box", [(-3.0, -1.0, -1.0, 1.0), (0.0, 10.0, 30.0, 40.0), (1.0, 1.05, -1.0, 1.0),
                                 (0.0, 10.0, -1.0, 1.0, 5.0, 9.0)])
def test_metric_box_empty_raises(box):
    with pytest.raises(ValueError):
        metric_box(box, KITTI_ORIGIN, 0.2, KITTI_GRID)


def test_region_need_bits():
    assert Region("a").need == 0 and Region("a").box is None
    assert Region("b", fov=True).need == hip.NEED_FOV
    assert Region("c", fov=True, masks=(0, 2)).need == 1 | 2 | 8
    with pytest.raises(ValueError):
        Region("d", masks=(3,))
    with pytest.raises(ValueError):
        Region("e", box=(0, 1, 0, 1))
    with pytest.raises(ValueError):
        SSCMetrics(4, regions=[Region("x"), Region("x")])
    with pytest.raises(ValueError):
        SSCMetrics(4, per_frame=True)


def test_kitti_preset_regions_of_the_model():
    """The `kitti` preset on config 2's geometry, and its refusal on another dataset (no model is built: the two methods
    only read a few attributes)."""
    from types import SimpleNamespace
    from occdepth_amd.models.OccDepth import OccDepth
    stub = SimpleNamespace(dataset="kitti", project_scale=2, full_scene_size=(256, 256, 32), REPORT_PRESETS=OccDepth.REPORT_PRESETS,
                           _kitti_origin=lambda batch=None: KITTI_ORIGIN)
    OccDepth.enable_eval_report(stub)
    regs = OccDepth._report_regions(stub, {})
    assert tuple(r.name for r in regs) == OccDepth.REPORT_PRESETS["kitti"]
    by = {r.name: r for r in regs}
    assert by["full"].box is None and not by["full"].fov and by["fov"].box is None and by["fov"].fov
    assert by["12.8m"].box == (0, 64, 96, 160, 0, 32) and by["25.6m"].box == (0, 128, 64, 192, 0, 32)
    assert by["fov_12.8m"].box == by["12.8m"].box and by["fov_12.8m"].fov and by["fov_25.6m"].box == by["25.6m"].box
    assert stub.eval_report["per_frame"] is False and stub.report_metrics == {}
    stub.dataset = "NYU"
    with pytest.raises(NotImplementedError, match="kitti"):
        OccDepth.enable_eval_report(stub, "kitti")
    with pytest.raises(ValueError):
        OccDepth.enable_eval_report(stub, "nuscenes")
    OccDepth.enable_eval_report(stub, [Region("full")])             # explicit regions work for any dataset
    assert OccDepth._report_regions(stub, {})[0].name == "full"


# ------------------------------------------------------------------------------------------------------- statistics
def test_region_stats_equal_reference_formulas():
    from oracle.losses import metrics_from_confusion
    g = np.random.default_rng(3)
    C = 7
    regs = [Region("full"), Region("near", box=(0, 2, 0, 2, 0, 2)), Region("dead", fov=True)]
    m = SSCMetrics(C, regions=regs)
    h = g.integers(0, 1000, size=(3, C, C))
    h[2] = 0                                               # an empty region: the reference's zero branch
    m.region_hist = torch.from_numpy(h)
    by_name = m.get_region_stats()
    assert list(by_name) == ["full", "near", "dead"]
    for i, r in enumerate(regs):
        ref = metrics_from_confusion(h[i])
        for got in (by_name[r.name], m.get_stats(region=r.name), m.get_stats(region=i), m.get_stats(region=r)):
            for k in ("precision", "recall", "iou", "iou_ssc_mean"):
                assert got[k] == ref[k], (r.name, k)
            assert np.array_equal(got["iou_ssc"], ref["iou_ssc"])
    assert by_name["dead"]["iou"] == 0 and by_name["dead"]["precision"] == 0
    with pytest.raises(KeyError):
        m.get_stats(region="nope")
    with pytest.raises(ValueError):
        SSCMetrics(C).get_stats(region=0)
    # per-frame blocks -> one dict per frame, in arrival order
    m.frame_hists = [torch.from_numpy(h[None]), torch.from_numpy(np.stack([h + 1, h + 2]))]
    fs = m.frame_stats()
    assert len(fs) == 3 and fs[2]["near"]["iou"] == metrics_from_confusion(h[1] + 2)["iou"]
    data_ptr = m.region_hist.data_ptr()
    m.reset()
    assert m.region_hist.data_ptr() == data_ptr and int(m.region_hist.abs().sum()) == 0 and m.frame_hists == []


# --------------------------------------------------------------------------------- the masked form, host side only
def _fake_regions(hist, target, regions, logits=None, labels=None, masks=(), fov=None, per_frame=False):
    """torch stand-in of hip.ssc_confusion_regions for byte masks and boxes (what the CPU tests of the class need)."""
    C = hist.shape[-1]
    B = target.shape[0]
    t = target.reshape(B, -1).long()
    p = (labels.reshape(B, -1).long() if labels is not None else logits.reshape(B, C, -1).argmax(1))
    have = [None if fov is None else fov.reshape(B, -1) != 0] + [m.reshape(B, -1) != 0 for m in masks]
    for r, (box, need) in enumerate(regions):
        keep = (t != 255) & (t < C) & (p < C)
        if box is not None:
            inside = torch.zeros(target.shape, dtype=torch.bool)
            inside[:, box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
            keep &= inside.reshape(B, -1)
        for bit in range(4):
            if need >> bit & 1:
                keep &= have[bit]
        for b in range(B):
            cnt = torch.bincount(t[b][keep[b]] * C + p[b][keep[b]], minlength=C * C).reshape(C, C)
            if per_frame:
                hist[b, r] += cnt
            else:
                hist[r] += cnt
    return hist


def _reference_masked_stats(pred, true, nonempty, nonsurface, C):
    """occdepth/loss/sscMetrics.py:70-109 restated: completion under labelled & nonempty & nonsurface, classes under
    labelled & nonempty."""
    lab = true != 255
    m_c = lab & (nonempty if nonempty is not None else True) & (nonsurface if nonsurface is not None else True)
    m_s = lab & (nonempty if nonempty is not None else True)
    bp, bt = pred[m_c] > 0, true[m_c] > 0
    tp, fp, fn = int((bt & bp).sum()), int((~bt & bp).sum()), int((bt & ~bp).sum())
    yp, yt = pred[m_s], true[m_s]
    tps = np.array([((yt == j) & (yp == j)).sum() for j in range(C)], dtype=np.float64)
    fps = np.array([((yt != j) & (yp == j)).sum() for j in range(C)], dtype=np.float64)
    fns = np.array([((yt == j) & (yp != j)).sum() for j in range(C)], dtype=np.float64)
    if tp != 0:
        precision, recall, iou = tp / (tp + fp), tp / (tp + fn), tp / (tp + fp + fn)
    else:
        precision, recall, iou = 0, 0, 0
    iou_ssc = tps / (tps + fps + fns + 1e-5)
    return {"precision": precision, "recall": recall, "iou": iou, "iou_ssc": iou_ssc, "iou_ssc_mean": np.mean(iou_ssc[1:])}


def _volumes(C=12, shape=(2, 5, 3, 4), seed=0):
    g = np.random.default_rng(seed)
    true = g.integers(0, C, size=shape).astype(np.uint8)
    true[g.random(shape) < 0.1] = 255
    pred = g.integers(0, C, size=shape).astype(np.uint8)
    return pred, true, g.random(shape) < 0.7, g.random(shape) < 0.6


@pytest.mark.parametrize("which", ["both", "nonempty", "nonsurface"])
def test_masked_add_batch_orchestration(monkeypatch, which):
    monkeypatch.setattr(hip, "ssc_confusion_regions", _fake_regions)
    C = 12
    pred, true, m1, m2 = _volumes(C)
    ne = m1 if which in ("both", "nonempty") else None
    ns = m2 if which in ("both", "nonsurface") else None
    m = SSCMetrics(C, device="cpu")
    m.add_batch(pred, true, nonempty=ne, nonsurface=None if ns is None else ns.reshape(2, -1).astype(np.uint8))
    m.add_batch(torch.from_numpy(pred), torch.from_numpy(true), nonempty=None if ne is None else torch.from_numpy(ne),
                nonsurface=None if ns is None else torch.from_numpy(ns))
    got = m.get_stats()
    ref = _reference_masked_stats(np.concatenate([pred, pred]), np.concatenate([true, true]),
                                  None if ne is None else np.concatenate([ne, ne]),
                                  None if ns is None else np.concatenate([ns, ns]), C)
    for k in ("precision", "recall", "iou", "iou_ssc_mean"):
        assert got[k] == ref[k], k
    assert np.array_equal(got["iou_ssc"], ref["iou_ssc"])
    assert m.hist is None and tuple(m.masked_hist.shape) == (2, C, C)


def test_mixing_masked_and_unmasked_raises(monkeypatch):
    import emu
    monkeypatch.setattr(hip, "ssc_confusion_regions", _fake_regions)
    C = 12
    pred, true, m1, m2 = _volumes(C)
    with emu.patched():
        m = SSCMetrics(C, device="cpu")
        m.add_batch(pred, true, nonempty=m1, nonsurface=m2)
        with pytest.raises(RuntimeError, match="reset"):
            m.add_batch(pred, true)
        with pytest.raises(RuntimeError, match="reset"):
            m.add_batch_logits(torch.randn(2, C, 5, 3, 4), torch.from_numpy(true))
        m.reset()
        m.add_batch(pred, true)                             # after reset() the other form is fine ...
        with pytest.raises(RuntimeError, match="reset"):
            m.add_batch(pred, true, nonempty=m1)            # ... and locks the object the other way round
    with pytest.raises(ValueError):
        SSCMetrics(C, regions=[Region("full")]).add_batch(pred, true, nonempty=m1)
    with pytest.raises(ValueError):
        SSCMetrics(C, device="cpu").add_batch(pred, true, masks=[m1])


def test_default_metric_still_uses_ssc_confusion(monkeypatch):
    """Constructed and called as before, the class goes through hip.ssc_confusion alone and keeps the (C, C) hist."""
    import emu

    def boom(*a, **k):
        raise AssertionError("the default path must not reach the region kernel")

    monkeypatch.setattr(hip, "ssc_confusion_regions", boom)
    C = 12
    pred, true, _, _ = _volumes(C)
    with emu.patched():
        calls = []
        inner = hip.ssc_confusion
        hip.ssc_confusion = lambda *a, **k: (calls.append(sorted(k)), inner(*a, **k))[1]
        try:
            m = SSCMetrics(C)
            m.device = torch.device("cpu")
            m.add_batch(pred, true)
            logits = torch.randn(2, C, 5, 3, 4)
            m.add_batch_logits(logits, torch.from_numpy(true))
        finally:
            hip.ssc_confusion = inner
    assert calls == [["labels"], ["logits"]]
    assert tuple(m.hist.shape) == (C, C) and m.hist.dtype == torch.int64 and m.region_hist is None and m.masked_hist is None
    lab = true != 255
    p2 = logits.reshape(2, C, -1).argmax(1).numpy().reshape(true.shape)
    want = np.bincount(C * true[lab].astype(np.int64) + pred[lab], minlength=C * C) + \
        np.bincount(C * true[lab].astype(np.int64) + p2[lab], minlength=C * C)
    assert np.array_equal(m.hist.numpy().reshape(-1), want)
    ptr = m.hist.data_ptr()
    m.reset()
    assert m.hist.data_ptr() == ptr and int(m.hist.sum()) == 0


# ------------------------------------------------------------------------------------------------------------ C ABI
def _valid_args():
    buf = (ctypes.c_double * 64)()
    ptr = (ctypes.addressof(buf) + 15) & ~15                # dummy address, never dereferenced: every call is rejected
    a = hip.ConfusionRegionsArgs()
    a.logits, a.target, a.hist = ptr, ptr, ptr
    a.batch, a.C, a.X, a.Y, a.Z, a.R = 2, 20, 8, 8, 4, 2
    a.s_b, a.s_c, a.s_v = 20 * 256, 256, 1
    for r in range(2):
        g = a.regions[r]
        g.x0, g.x1, g.y0, g.y1, g.z0, g.z1 = 0, 8, 0, 8, 0, 4
    return a, ptr, buf


def _set(path, value):
    def edit(a, ptr):
        obj = a
        *head, last = path
        for step in head:
            obj = obj[step] if isinstance(step, int) else getattr(obj, step)
        if isinstance(last, int):
            obj[last] = value(ptr) if callable(value) else value
        else:
            setattr(obj, last, value(ptr) if callable(value) else value)
    return edit


def _fov_by_calibration(**over):
    def edit(a, ptr):
        a.regions[1].need = hip.NEED_FOV
        a.cam_E = a.cam_k = ptr
        a.n_views, a.view_mask, a.img_w, a.img_h, a.voxel_size = 2, 1, 320, 96, 0.2
        for k, v in over.items():
            setattr(a, k, v)
    return edit


INVALID = {
    "both predictions": _set(("labels",), lambda p: p),
    "no prediction": _set(("logits",), None),
    "no target": _set(("target",), None),
    "no hist": _set(("hist",), None),
    "R = 0": _set(("R",), 0),
    "R = 9": _set(("R",), 9),
    "empty box": _set(("regions", 1, "x1"), 0),
    "reversed box": _set(("regions", 0, "z0"), 4),
    "box past the grid": _set(("regions", 1, "y1"), 9),
    "negative box": _set(("regions", 0, "x0"), -1),
    "mask bit without mask": _set(("regions", 1, "need"), hip.NEED_MASK0 << 1),
    "FOV bit without a source": _set(("regions", 0, "need"), hip.NEED_FOV),
    "unknown need bit": _set(("regions", 0, "need"), 16),
    "C = 0": _set(("C",), 0),
    "C = 33": _set(("C",), 33),
    "negative frame stride": _set(("frame_stride",), -1),
    "frame stride below R*C*C": _set(("frame_stride",), 2 * 20 * 20 - 1),
    "V = 0": _fov_by_calibration(n_views=0),
    "V = 5": _fov_by_calibration(n_views=5, view_mask=1),
    "no view selected": _fov_by_calibration(view_mask=0),
    "view outside V": _fov_by_calibration(view_mask=4),
    "cam_k missing": _fov_by_calibration(cam_k=None),
    "two FOV sources": lambda a, ptr: (_fov_by_calibration()(a, ptr), setattr(a, "fov", ptr)),
    "empty grid": _set(("Z",), 0),
}


@pytest.mark.parametrize("case", list(INVALID))
def test_confusion_regions_rejects_before_launch(hip_lib, case):
    a, ptr, buf = _valid_args()
    INVALID[case](a, ptr)
    assert hip_lib.occd_ssc_confusion_regions(ctypes.byref(a), None) == -1, case


def test_confusion_regions_rejects_null_and_lds_bound(hip_lib):
    assert hip_lib.occd_ssc_confusion_regions(None, None) == -1
    a, ptr, buf = _valid_args()
    a.C, a.R = 46, 8                                         # 8 * 46 * 46 * 4 bytes of counters > 64 KiB (and C > 32)
    assert hip_lib.occd_ssc_confusion_regions(ctypes.byref(a), None) == -1
    assert hip.ABI_VERSION == 22 and hip_lib.occd_abi_version() == 22


def test_confusion_regions_struct_layout(tmp_path):
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "occdepth_amd.h")
    structs = {"occd_confusion_region": hip.ConfusionRegion, "occd_confusion_regions_args": hip.ConfusionRegionsArgs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, st in structs.items():
        assert int(out[cname]) == ctypes.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(st, fname).offset, f"{cname}.{fname}"
    assert hip.MAX_REGIONS == 8
