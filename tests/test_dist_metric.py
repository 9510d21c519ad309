"""CPU: the numpy restatements of K37 (dist_metric.edt_sq_ref, dist_metric_ref) against brute force and analytic cases,
DistanceMetrics and the model hook on a Python stand-in for the kernel, the offline tool, and the entry points' argument
checks (no launch).  tests/test_dist_metric_gpu.py holds the kernels to the restatements."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from occdepth_amd import dist_metric as dm
from occdepth_amd import hip
from test_map import HOOK_C, HOOK_DIMS, _confusion_stand_in, _hook_steps, _hook_stub


# ----------------------------------------------------------------------------------------------------- volumes
def random_labels(shape, C, seed, p_occ=0.15, junk=True):
    """(B, X, Y, Z) uint8: class 0 mostly, classes 1 .. C - 1 with probability p_occ, and -- with junk -- a sprinkle of
    labels >= C and 255, which are no seeds."""
    g = np.random.default_rng(seed)
    lab = np.where(g.random(shape) < p_occ, g.integers(1, C, shape), 0).astype(np.uint8)
    if junk:
        r = g.random(shape)
        lab[r < 0.03] = 255
        lab[(r >= 0.03) & (r < 0.05)] = C + 1
    return lab


def brute_force(labels, slot, C, T):
    """All-pairs minimum of one (X, Y, Z) volume -> (X, Y, Z) int64."""
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in labels.shape], indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    seeds = idx[dm.seeds_of(labels, slot, C).reshape(-1)]
    if len(seeds) == 0:
        return np.full(labels.shape, T + 1, dtype=np.int64)
    d = ((idx[:, None, :] - seeds[None, :, :]) ** 2).sum(-1).min(1)
    return np.minimum(d, T + 1).reshape(labels.shape)


# ----------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape,C,T", [((2, 19, 13, 7), 5, 1024), ((1, 40, 9, 5), 4, 16), ((1, 12, 12, 12), 3, 65534),
                                       ((1, 30, 5, 11), 6, 7)])
def test_edt_ref_equals_brute_force(shape, C, T):
    lab = random_labels(shape, C, sum(shape) + T, p_occ=0.04)
    slots = list(range(C))
    got = dm.edt_sq_ref(lab, slots, C, T)
    assert got.dtype == np.uint16 and got.shape == (shape[0], C) + shape[1:]
    for b in range(shape[0]):
        for s in slots:
            assert np.array_equal(got[b, s], brute_force(lab[b], s, C, T)), (b, s)
    if T <= 16:
        assert got.max() == T + 1                                           # the truncation bites where it can


def test_edt_ref_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    C, T = 5, 100
    lab = random_labels((1, 64, 64, 16), C, 3, p_occ=0.002)
    got = dm.edt_sq_ref(lab, [0, 2], C, T)
    for i, s in enumerate((0, 2)):
        seeds = dm.seeds_of(lab[0], s, C)
        assert seeds.any()
        want = np.minimum(np.rint(ndi.distance_transform_edt(~seeds) ** 2), T + 1).astype(np.int64)
        assert np.array_equal(got[0, i], want)
    assert (got == T + 1).any() and (got == 0).any()


def test_single_seed_in_a_corner_and_no_seed():
    dims, C, T = (9, 8, 7), 4, 50
    lab = np.zeros((1,) + dims, dtype=np.uint8)
    lab[0, 0, 0, 0] = 2
    x, y, z = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    want = np.minimum(x * x + y * y + z * z, T + 1)
    got = dm.edt_sq_ref(lab, [0, 2, 1], C, T)
    assert np.array_equal(got[0, 0], want) and np.array_equal(got[0, 1], want)
    assert (got[0, 2] == T + 1).all()                                       # an empty slot: T + 1 everywhere
    lab[0, 0, 0, 0] = 4                                                     # a label >= C is no seed of slot 0 either
    assert (dm.edt_sq_ref(lab, [0], C, T) == T + 1).all()
    lab[0, 0, 0, 0] = 255
    assert (dm.edt_sq_ref(lab, [0], C, T) == T + 1).all()
    wide = np.zeros((1,) + dims, dtype=np.uint16)                           # 16-bit labels: 258 is not class 2
    wide[0, 0, 0, 0] = 258
    assert (dm.edt_sq_ref(wide, [0, 2], C, T) == T + 1).all()
    assert (dm.edt_sq_ref(torch.from_numpy(wide.view(np.int16)), [0, 2], C, T) == T + 1).all()


def counts3(c, C, T):
    return np.asarray(c).reshape(2, C, T + 2)


def test_identical_volumes_put_all_mass_in_bin_zero():
    C, T = 5, 64
    lab = random_labels((2, 10, 9, 8), C, 5, junk=False)
    c = counts3(dm.dist_metric_ref(lab, lab, None, C, T), C, T)
    assert not c[:, :, 1:].any()
    occ = (lab >= 1) & (lab < C)
    assert c[0, 0, 0] == c[1, 0, 0] == occ.sum() > 0
    for cl in range(1, C):
        assert c[0, cl, 0] == c[1, cl, 0] == (lab == cl).sum() > 0
    m = dm.DistanceMetrics(C, 0.2, max_d2=T).merge_(torch.from_numpy(c.reshape(-1)))
    s = m.get_stats()
    assert (s["F"] == 1.0).all() and (s["precision"] == 1.0).all() and (s["recall"] == 1.0).all()
    assert s["CD_geo"] == 0.0 and s["CD_sem"] == 0.0 and not s["CD"].any() and not s["overflow"].any()
    assert (s["F_sem"] == 1.0).all() and (s["F_geo"] == 1.0).all()


def test_prediction_shifted_by_one_voxel_along_x():
    """A wall at x = 5 predicted at x = 6: every voxel of either is at squared distance 1 of the other."""
    C, T, dims = 4, 64, (12, 6, 5)
    target = np.zeros((1,) + dims, dtype=np.uint8)
    target[0, 5] = 2
    pred = np.roll(target, 1, axis=1)
    c = counts3(dm.dist_metric_ref(pred, target, None, C, T), C, T)
    n = dims[1] * dims[2]
    for side in (0, 1):
        for s in (0, 2):
            want = np.zeros(T + 2, dtype=np.int64)
            want[1] = n
            assert np.array_equal(c[side, s], want)
        assert not c[side, 1].any() and not c[side, 3].any()
    s = dm.DistanceMetrics(C, 0.2, thresholds_m=(0.1, 0.2, 0.4), max_d2=T).merge_(torch.from_numpy(c.reshape(-1))).get_stats()
    assert s["bins"] == (0, 1, 4)
    assert s["F_geo"].tolist() == [0.0, 1.0, 1.0] and s["F_sem"].tolist() == [0.0, 1.0, 1.0]
    assert np.isclose(s["CD_geo"], 0.4) and np.isclose(s["CD_sem"], 0.4) and s["present"].tolist() == [False, False, True, False]
    # voxel IoU of the same pair is 0: that is the point of the metric
    assert not ((pred > 0) & (target > 0)).any()


def test_empty_slot_class_in_one_volume_only_unknown_and_mask():
    C, T, dims = 5, 20, (8, 7, 6)
    target = np.zeros((1,) + dims, dtype=np.uint8)
    pred = np.zeros((1,) + dims, dtype=np.uint8)
    target[0, 2, 2, 2] = 1
    pred[0, 2, 2, 4] = 1                       # class 1 in both, squared distance 4
    target[0, 6, 6, 5] = 3                     # class 3 only in the target: its voxel finds no class-3 prediction
    pred[0, 0, 0, 0] = 4                       # class 4 only in the prediction
    c = counts3(dm.dist_metric_ref(pred, target, None, C, T), C, T)
    assert c[0, 1, 4] == 1 and c[1, 1, 4] == 1 and c[0, 1].sum() == 1
    assert c[1, 3, T + 1] == 1 and c[1, 3].sum() == 1 and not c[0, 3].any()          # no seed at all: the overflow bin
    assert c[0, 4, T + 1] == 1 and not c[1, 4].any()
    assert not c[:, 2].any()                                                          # the empty slot
    assert c[0, 0].sum() == 2 and c[1, 0].sum() == 2
    # slot 0 of the target voxel (6, 6, 5): the nearest prediction of any class is (2, 2, 4): 16 + 16 + 1 = 33 > T
    assert c[1, 0, T + 1] == 1 and c[1, 0, 4] == 1
    s = dm.DistanceMetrics(C, 0.2, thresholds_m=(0.4,), max_d2=T).merge_(torch.from_numpy(c.reshape(-1))).get_stats()
    assert s["present"].tolist() == [False, True, False, True, False]
    assert s["F"][0].tolist() == [0.5, 1.0, 0.0, 0.0, 0.0] and s["F_sem"][0] == 0.5   # class 4 has no target query: left out
    assert np.isclose(s["CD"][3], 0.2 * np.sqrt(T + 1)) and s["overflow"][1, 3] == 1.0 and s["overflow_geo"].tolist() == [0.0, 0.5]
    # queries are restricted, seeds are not: the target voxel next to an unknown region is still recalled by a prediction inside it
    target[0, 2, 2, 4] = 255
    c = counts3(dm.dist_metric_ref(pred, target, None, C, T), C, T)
    assert c[0, 1].sum() == 0 and c[1, 1, 4] == 1
    mask = np.ones((1,) + dims, dtype=np.uint8)
    mask[0, 2, 2, 2] = 0
    c = counts3(dm.dist_metric_ref(pred, target, mask, C, T), C, T)
    assert not c[:, 1].any() and c[1, 3, T + 1] == 1
    assert not dm.dist_metric_ref(pred, target, np.zeros_like(mask), C, T).any()


def test_fused_count_equals_edt_then_counting():
    C, T = 5, 3
    pred, target = random_labels((2, 9, 8, 7), C, 1), random_labels((2, 9, 8, 7), C, 2)
    mask = np.random.default_rng(3).random(pred.shape) < 0.7
    c = counts3(dm.dist_metric_ref(pred, target, mask, C, T), C, T)
    query = (target != 255) & mask
    Dt, Dp = dm.edt_sq_ref(target, range(C), C, T), dm.edt_sq_ref(pred, range(C), C, T)
    for s in range(C):
        assert np.array_equal(c[0, s], np.bincount(Dt[:, s][query & dm.seeds_of(pred, s, C)], minlength=T + 2))
        assert np.array_equal(c[1, s], np.bincount(Dp[:, s][query & dm.seeds_of(target, s, C)], minlength=T + 2))
    assert c[:, :, 1:T + 1].any() and c[:, :, T + 1].any() and c[:, :, 0].any()


# ----------------------------------------------------------------------------------------------------- the kernel stand-in
class DistStandIn:
    """hip.dist_metric on CPU tensors, from what the host side hands over."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "dist_metric", self.dist_metric)
        return self

    def dist_metric(self, pred, target, counts, n_classes, max_d2, scratch, mask=None):
        for t in (pred, target):
            assert t.dim() == 4 and t.is_contiguous() and t.dtype in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16))
        assert target.shape == pred.shape and counts.dtype == torch.int64 and counts.numel() == hip.dist_metric_size(n_classes, max_d2)
        assert scratch.numel() * scratch.element_size() >= hip.dist_metric_scratch_bytes(pred.shape[1:])
        assert mask is None or (mask.shape == pred.shape and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous())
        self.calls.append({"batch": int(pred.shape[0]), "dtypes": (pred.dtype, target.dtype), "mask": None if mask is None else mask.clone(),
                           "pred": pred.clone(), "max_d2": max_d2})
        counts += torch.from_numpy(dm.dist_metric_ref(pred, target, mask, n_classes, max_d2))
        return counts


def test_distance_metrics_on_the_stand_in(monkeypatch):
    k = DistStandIn().install(monkeypatch)
    C, T = 5, 40
    pa, ta = random_labels((1, 9, 8, 7), C, 1), random_labels((1, 9, 8, 7), C, 2)
    pb, tb = random_labels((2, 9, 8, 7), C, 3), random_labels((2, 9, 8, 7), C, 4)
    m = dm.DistanceMetrics(C, 0.2, max_d2=T)
    assert m.size == 2 * C * (T + 2) == hip.dist_metric_size(C, T) and m.counts().tolist() == [0] * m.size and m.scratch_bytes() == 0
    assert m.bins == (1, 4, 16)                                             # 0.2 / 0.4 / 0.8 m at 0.2 m
    assert m.add_batch(torch.from_numpy(pa), torch.from_numpy(ta)) is m
    first = dm.dist_metric_ref(pa, ta, None, C, T)
    assert np.array_equal(m.counts().numpy(), first)
    assert m.scratch_bytes() == hip.dist_metric_scratch_bytes((9, 8, 7)) == 32 * 9 * 8 * 7
    # a second batch: wider labels are narrowed, a bool mask goes through, the counters accumulate
    mask = torch.from_numpy(np.random.default_rng(5).random(pb.shape) < 0.6)
    m.add_batch(torch.from_numpy(pb.astype(np.int64)), torch.from_numpy(tb.astype(np.int32)), mask.reshape(2, -1))
    assert k.calls[-1]["dtypes"] == (torch.int16, torch.int16) and k.calls[-1]["batch"] == 2 and k.calls[-1]["max_d2"] == T
    second = dm.dist_metric_ref(pb, tb, mask.numpy(), C, T)
    total = first + second
    assert np.array_equal(m.counts().numpy(), total) and second.any()
    # statistics: the arithmetic restated from the counters
    s, c = m.get_stats(), counts3(total, C, T).astype(np.float64)
    root = np.sqrt(np.arange(T + 2))
    for i, kbin in enumerate(m.bins):
        for sl in range(C):
            P = c[0, sl, :kbin + 1].sum() / c[0, sl].sum()
            R = c[1, sl, :kbin + 1].sum() / c[1, sl].sum()
            assert s["precision"][i, sl] == P and s["recall"][i, sl] == R
            assert np.isclose(s["F"][i, sl], 2 * P * R / (P + R) if P + R else 0.0, rtol=1e-14, atol=0)
        assert s["F_geo"][i] == s["F"][i, 0] and np.isclose(s["F_sem"][i], s["F"][i, 1:].mean(), rtol=1e-14, atol=0)
    cd = [0.2 * ((c[0, sl] * root).sum() / c[0, sl].sum() + (c[1, sl] * root).sum() / c[1, sl].sum()) for sl in range(C)]
    assert np.allclose(s["CD"], cd, rtol=1e-14, atol=0) and s["CD_geo"] == s["CD"][0] and np.isclose(s["CD_sem"], np.mean(cd[1:]))
    assert 0.0 < s["F_geo"][0] < s["F_geo"][2] <= 1.0 and s["CD_geo"] > 0.0
    assert np.array_equal(s["overflow"], c[:, :, T + 1] / c.sum(2)) and np.isclose(s["truncation_m"], 0.2 * np.sqrt(T + 1))
    # merge_ and reset
    other = dm.DistanceMetrics(C, 0.2, max_d2=T).add_batch(torch.from_numpy(pa), torch.from_numpy(ta))
    assert torch.equal(m.merge_(other).counts(), torch.from_numpy(total + first))
    assert m.reset() is m and not m.counts().any()
    with pytest.raises(ValueError):
        m.merge_(torch.zeros(5, dtype=torch.int64))


def test_statistics_from_hand_made_counters():
    C, T = 4, 9
    m = dm.DistanceMetrics(C, 0.5, thresholds_m=(0.5, 1.0), max_d2=T)
    assert m.bins == (1, 4)
    c = np.zeros((2, C, T + 2), dtype=np.int64)
    c[0, 0, [0, 1, 4, 10]] = [10, 20, 30, 40]                              # 100 predicted occupied voxels
    c[1, 0, [0, 2, 9]] = [25, 25, 50]                                      # 100 true ones
    c[0, 1, 0], c[1, 1, 0] = 8, 4                                          # class 1: perfect
    c[0, 2, 10] = 5                                                        # class 2: predicted, never true -> not present
    c[1, 3, 3] = 6                                                         # class 3: true, never predicted near
    s = m.merge_(torch.from_numpy(c.reshape(-1))).get_stats()
    assert s["precision_geo"].tolist() == [0.3, 0.6] and s["recall_geo"].tolist() == [0.25, 0.5]
    assert np.allclose(s["F_geo"], [2 * 0.3 * 0.25 / 0.55, 2 * 0.6 * 0.5 / 1.1])
    assert s["present"].tolist() == [False, True, False, True]
    assert s["F"][:, 1].tolist() == [1.0, 1.0] and s["F"][:, 2].tolist() == [0.0, 0.0]
    assert s["precision"][:, 3].tolist() == [0.0, 0.0] and s["recall"][:, 3].tolist() == [0.0, 1.0] and s["F"][:, 3].tolist() == [0.0, 0.0]
    assert s["F_sem"].tolist() == [0.5, 0.5]
    side0 = (20 * 1 + 30 * 2 + 40 * np.sqrt(10)) / 100
    side1 = (25 * np.sqrt(2) + 50 * 3) / 100
    assert np.isclose(s["CD_geo"], 0.5 * (side0 + side1))
    assert np.isclose(s["CD"][3], 0.5 * np.sqrt(3)) and np.isclose(s["CD_sem"], (0.0 + 0.5 * np.sqrt(3)) / 2)
    assert s["overflow_geo"].tolist() == [0.4, 0.0] and s["overflow"][0, 2] == 1.0
    assert s["queries"].tolist() == [[100, 8, 5, 0], [100, 4, 0, 6]]
    empty = dm.DistanceMetrics(C, 0.5, thresholds_m=(0.5,), max_d2=T).get_stats()
    assert empty["F_geo"].tolist() == [0.0] and empty["F_sem"].tolist() == [0.0] and empty["CD_geo"] == 0.0 and empty["CD_sem"] == 0.0


def test_thresholds_and_refusals():
    assert dm.threshold_bins((0.2, 0.4, 0.8), 0.2, 1024) == (1, 4, 16)
    assert dm.threshold_bins((0.3, 0.6, 6.4), 0.2, 1024) == (2, 9, 1024)     # 1.5^2 = 2.25 -> 2; 0.6 / 0.2 is 2.9999.. in floats
    assert dm.threshold_bins((0.08, 0.1), 0.08, 10) == (1, 1)
    with pytest.raises(ValueError, match="max_d2"):
        dm.threshold_bins((6.6,), 0.2, 1024)                                 # 33^2 = 1089 > 1024
    with pytest.raises(ValueError, match="max_d2"):
        dm.DistanceMetrics(20, 0.2, thresholds_m=(1.0,), max_d2=24)          # k = 25 > T
    dm.DistanceMetrics(20, 0.2, thresholds_m=(1.0,), max_d2=25)
    with pytest.raises(ValueError, match="n_classes"):
        dm.DistanceMetrics(33, 0.2)
    with pytest.raises(ValueError, match="max_d2"):
        dm.DistanceMetrics(20, 0.2, max_d2=65535)
    with pytest.raises(ValueError, match="threshold"):
        dm.DistanceMetrics(20, 0.2, thresholds_m=())
    with pytest.raises(ValueError, match="voxel_size"):
        dm.DistanceMetrics(20, 0.0)
    m = dm.DistanceMetrics(20, 0.2)
    lab = torch.zeros((1, 4, 3, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match="integer"):
        m.add_batch(lab.float(), lab)
    with pytest.raises(ValueError, match="shape"):
        m.add_batch(lab, lab[:, :2])
    with pytest.raises(ValueError, match="mask"):
        m.add_batch(lab, lab, torch.zeros(5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="GPU"):                           # no CPU path behind the binding
        m.add_batch(lab, lab)
    counts = torch.zeros(hip.dist_metric_size(20, 1024), dtype=torch.int64)
    scratch = torch.zeros(hip.dist_metric_scratch_bytes((4, 3, 2)), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="B, X, Y, Z"):
        hip.dist_metric(lab[0], lab[0], counts, 20, 1024, scratch)
    with pytest.raises(RuntimeError, match="counters"):
        hip.dist_metric(lab, lab, counts[:-1], 20, 1024, scratch)
    with pytest.raises(RuntimeError, match="scratch"):
        hip.dist_metric(lab, lab, counts, 20, 1024, scratch[:-1])
    with pytest.raises(RuntimeError, match="max_d2"):
        hip.dist_metric(lab, lab, counts[:hip.dist_metric_size(20, 0)], 20, 0, scratch)
    with pytest.raises(RuntimeError, match="n_classes"):
        hip.dist_metric(lab, lab, torch.zeros(hip.dist_metric_size(33, 1024), dtype=torch.int64), 33, 1024, scratch)
    with pytest.raises(RuntimeError, match="mask"):
        hip.dist_metric(lab, lab, counts, 20, 1024, scratch, mask=lab.float())
    with pytest.raises(RuntimeError, match="slots"):
        hip.edt_sq(lab, [], 20, 1024)
    with pytest.raises(RuntimeError, match="slots"):
        hip.edt_sq(lab, [20], 20, 1024)
    with pytest.raises(RuntimeError, match="GPU"):
        hip.edt_sq(lab, [0], 20, 1024)


# ----------------------------------------------------------------------------------------------------- the model hook
def _install(monkeypatch):
    k = DistStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    return k


def _dist_stub(**extra):
    from occdepth_amd.models.OccDepth import OccDepth
    stub = _hook_stub(**extra)
    stub._dist_epoch_end = lambda step_type: OccDepth._dist_epoch_end(stub, step_type)
    return stub


def _epoch(stub, step_type, steps, fused=None):
    """What step() and the epoch end do with the ordinary metric and the distance pass."""
    from occdepth_amd.models.OccDepth import OccDepth
    metric = getattr(stub, step_type + "_metrics")
    for n, (batch, logits, target) in enumerate(steps):
        metric.add_batch_logits(logits, target)
        if getattr(stub, "dist_metrics", None) is not None:
            OccDepth._dist_step(stub, step_type, batch, logits, target, None if fused is None else fused[n])
    (OccDepth.validation_epoch_end if step_type == "val" else OccDepth.test_epoch_end)(stub, [])


def _hook_reference(steps, T, labels=None, fov=False):
    total = 0
    for n, (batch, logits, target) in enumerate(steps):
        pred = logits.argmax(1).numpy() if labels is None else labels[n].numpy()
        mask = torch.stack(batch["fov_mask_1"]).reshape(target.shape).numpy() if fov else None
        total = total + dm.dist_metric_ref(pred, target.numpy(), mask, HOOK_C, T)
    return total


def test_model_hook_logs_and_prints(monkeypatch, capsys):
    from occdepth_amd.models.OccDepth import OccDepth
    k = _install(monkeypatch)
    steps = _hook_steps()

    # off: a stub WITHOUT the attribute, as the existing hook tests build it -- no key, no line, no launch
    plain = _hook_stub()
    _epoch(plain, "val", steps)
    capsys.readouterr()
    _epoch(plain, "test", steps)
    lines_off = capsys.readouterr().out.splitlines()
    assert not k.calls and not any("dist" in key.lower() for key in plain.logged_keys) and not any("dist" in l for l in lines_off)

    stub = _dist_stub(dist_metrics=None)
    assert OccDepth.enable_distance_metrics(stub) is stub
    assert stub.dist_metrics["thresholds_m"] == (0.2, 0.4, 0.8) and stub.dist_metrics["max_d2"] == 1024 and not stub.dist_metrics["fov_only"]
    _epoch(stub, "val", steps)
    new = set(stub.logged_keys) - set(plain.logged_keys)
    assert new == {"val_dist/F_geo@0.2", "val_dist/F_geo@0.4", "val_dist/F_geo@0.8", "val_dist/F_sem@0.2", "val_dist/F_sem@0.4",
                   "val_dist/F_sem@0.8", "val_dist/CD_geo", "val_dist/CD_sem"}
    assert all(np.array_equal(stub.logged_keys[key], plain.logged_keys[key]) for key in plain.logged_keys)
    assert [c["batch"] for c in k.calls] == [2, 1, 1] and all(c["mask"] is None for c in k.calls)      # one call per step
    want = _hook_reference(steps, 1024)
    ref = dm.DistanceMetrics(HOOK_C, 0.2).merge_(torch.from_numpy(want)).get_stats()
    assert ref["queries"][:, 0].min() > 0
    assert stub.logged_keys["val_dist/F_geo@0.4"] == ref["F_geo"][1] and stub.logged_keys["val_dist/F_sem@0.2"] == ref["F_sem"][0]
    assert stub.logged_keys["val_dist/CD_geo"] == ref["CD_geo"] and stub.logged_keys["val_dist/CD_sem"] == ref["CD_sem"]
    assert 0.0 < ref["F_geo"][0] <= ref["F_geo"][2] <= 1.0
    assert not stub.dist_metrics["metrics"]["val"].counts().any()            # reset for the next epoch

    capsys.readouterr()
    _epoch(stub, "test", steps)
    lines = capsys.readouterr().out.splitlines()
    assert lines[:len(lines_off)] == lines_off
    block = lines[len(lines_off):]
    assert block[0] == "test_dist======"
    assert block[1].startswith("@0.2m: F_geo=%.4f, Precision_geo=" % (ref["F_geo"][0] * 100)) and "F_sem=" in block[1]
    assert [l.split(":")[0] for l in block[1:4]] == ["@0.2m", "@0.4m", "@0.8m"]
    assert block[4].startswith("CD_geo=%.4f m, CD_sem=%.4f m (truncated at 6.40 m" % (ref["CD_geo"], ref["CD_sem"]))
    assert block[5].startswith("class F / CD: ['0', '1', '2', '3']")
    assert [l.split(":")[0] for l in block[6:]] == ["F@0.2m", "F@0.4m", "F@0.8m", "CD[m]"] and len(block) == 10

    # the fused labels go into a second metric; fov_only hands the batch's FOV mask over as the query mask
    fused = [torch.roll(logits.argmax(1), 1, dims=1).to(torch.uint8) for _, logits, _ in steps]
    both = OccDepth.enable_distance_metrics(_dist_stub(dist_metrics=None), thresholds_m=(0.2, 1.0), max_d2=30, fov_only=True)
    k.calls.clear()
    _epoch(both, "val", steps, fused)
    assert len(k.calls) == 6 and all(c["mask"] is not None and c["max_d2"] == 30 for c in k.calls)
    assert torch.equal(k.calls[0]["mask"].bool(), torch.stack(steps[0][0]["fov_mask_1"]).reshape(steps[0][2].shape))
    assert {key for key in both.logged_keys if "fused_dist" in key} == {
        "val_fused_dist/F_geo@0.2", "val_fused_dist/F_geo@1", "val_fused_dist/F_sem@0.2", "val_fused_dist/F_sem@1",
        "val_fused_dist/CD_geo", "val_fused_dist/CD_sem"}
    ref_p = dm.DistanceMetrics(HOOK_C, 0.2, (0.2, 1.0), 30).merge_(torch.from_numpy(_hook_reference(steps, 30, fov=True))).get_stats()
    ref_f = dm.DistanceMetrics(HOOK_C, 0.2, (0.2, 1.0), 30).merge_(torch.from_numpy(_hook_reference(steps, 30, fused, fov=True))).get_stats()
    assert both.logged_keys["val_dist/F_geo@1"] == ref_p["F_geo"][1] and both.logged_keys["val_fused_dist/F_geo@1"] == ref_f["F_geo"][1]
    assert both.logged_keys["val_fused_dist/CD_geo"] == ref_f["CD_geo"] != both.logged_keys["val_dist/CD_geo"]
    assert ref_p["queries"][0, 0] < ref["queries"][0, 0]                     # the mask took queries away
    capsys.readouterr()
    _epoch(both, "test", steps, fused)
    out = capsys.readouterr().out.splitlines()
    assert out.count("test_dist======") == 1 and out.count("test_fused_dist======") == 1

    # not restricted to SemanticKITTI: the voxel size is the dataset's
    nyu = OccDepth.enable_distance_metrics(_dist_stub(dataset="NYU", dist_metrics=None), thresholds_m=(0.08,))
    _epoch(nyu, "val", steps)
    assert nyu.logged_keys["val_dist/F_geo@0.08"] == ref["F_geo"][0]         # one voxel, whatever it measures
    assert np.isclose(nyu.logged_keys["val_dist/CD_geo"], ref["CD_geo"] * 0.08 / 0.2)
    # refusals
    with pytest.raises(ValueError, match="threshold"):
        OccDepth.enable_distance_metrics(_dist_stub(dist_metrics=None), thresholds_m=())
    with pytest.raises(ValueError, match="max_d2"):
        OccDepth.enable_distance_metrics(_dist_stub(dist_metrics=None), max_d2=0)
    late = OccDepth.enable_distance_metrics(_dist_stub(dist_metrics=None), thresholds_m=(7.0,))
    with pytest.raises(ValueError, match="max_d2"):                          # k = 1225 > 1024: refused with the first batch
        OccDepth._dist_step(late, "val", *steps[0])
    nofov = OccDepth.enable_distance_metrics(_dist_stub(dist_metrics=None), fov_only=True)
    k.calls.clear()
    with pytest.raises(ValueError, match="fov_mask_1"):
        OccDepth._dist_step(nofov, "val", {"sequence": ["08"], "frame_id": ["000000"]}, steps[0][1][:1], steps[0][2][:1])
    assert not k.calls


def test_allreduce_sums_the_counters_over_the_ranks(monkeypatch):
    from types import SimpleNamespace
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

    m = dm.DistanceMetrics(HOOK_C, 0.2, thresholds_m=(0.2,), max_d2=8)
    m.merge_(torch.arange(m.size, dtype=torch.int64))
    assert m.allreduce_(TwoRanks) is m and torch.equal(m.counts(), 2 * torch.arange(m.size)) and TwoRanks.calls == 1
    seen = []
    monkeypatch.setattr(dm.DistanceMetrics, "allreduce_", lambda self, dist=None: seen.append(self) or self)
    for flag in (False, True):
        stub = OccDepth.enable_distance_metrics(_dist_stub(dist_metrics=None))
        stub.metrics_allreduce = flag
        _epoch(stub, "val", steps)
        assert len(seen) == int(flag)


def test_distance_metrics_are_switched_by_the_environment(monkeypatch):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def state():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg).dist_metrics

    for var in ("OCCDEPTH_DIST_METRIC", "OCCDEPTH_DIST_THRESHOLDS", "OCCDEPTH_DIST_FOV", "OCCDEPTH_RAY_METRIC", "OCCDEPTH_FUSE",
                "OCCDEPTH_MAP_DIR"):
        monkeypatch.delenv(var, raising=False)
    assert state() is None
    monkeypatch.setenv("OCCDEPTH_DIST_THRESHOLDS", "0.5")                    # without the switch: nothing
    assert state() is None
    monkeypatch.delenv("OCCDEPTH_DIST_THRESHOLDS")
    monkeypatch.setenv("OCCDEPTH_DIST_METRIC", "1")
    st = state()
    assert (st["thresholds_m"], st["max_d2"], st["fov_only"]) == ((0.2, 0.4, 0.8), 1024, False)
    monkeypatch.setenv("OCCDEPTH_DIST_THRESHOLDS", "0.5,1,2.5")
    monkeypatch.setenv("OCCDEPTH_DIST_FOV", "1")
    st = state()
    assert (st["thresholds_m"], st["fov_only"]) == ((0.5, 1.0, 2.5), True)
    monkeypatch.setenv("OCCDEPTH_DIST_THRESHOLDS", "0.5,x")
    with pytest.raises(ValueError, match="OCCDEPTH_DIST_THRESHOLDS"):
        state()


def test_off_imports_nothing():
    """With the feature off the model module does not import occdepth_amd.dist_metric (checked in a fresh interpreter)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); import occdepth_amd.models.OccDepth; "
            "assert 'occdepth_amd.dist_metric' not in sys.modules; print('clean')" % root)
    env = {k: v for k, v in os.environ.items() if not k.startswith("OCCDEPTH_DIST")}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "clean", out.stderr


# ----------------------------------------------------------------------------------------------------- the offline tool
def _tool():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "dist_metric.py")
    spec = importlib.util.spec_from_file_location("dist_metric_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dist_metric_tool_scores_saved_volumes(monkeypatch, tmp_path, capsys):
    tool = _tool()
    k = _install(monkeypatch)
    dims, C = (10, 9, 6), 20
    pred_dir, gt_dir = tmp_path / "predictions", tmp_path / "gt"
    os.makedirs(pred_dir)
    os.makedirs(gt_dir)
    frames = []
    for n in range(2):
        target = random_labels(dims, C, 30 + n, junk=False)
        target[0, 0, n] = 255
        pred = np.roll(target, 1, axis=0)
        pred[pred == 255] = 0
        frames.append((pred, target))
        with open(pred_dir / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": pred.astype(np.uint16)}, f)
        with open(gt_dir / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"target": target.astype(np.uint16)}, f)
    with open(pred_dir / "000007.pkl", "wb") as f:                           # no target for it: not scored
        pickle.dump({"y_pred": frames[0][0].astype(np.uint16)}, f)
    base = ["--pred", str(pred_dir), "--gt", str(gt_dir), "--dims", "10", "9", "6"]
    args = tool.parser().parse_args(base)
    assert (args.classes, tuple(args.thresholds), args.max_d2, args.voxel_size) == (20, (0.2, 0.4, 0.8), 1024, 0.2)
    stats = tool.run(args, device=torch.device("cpu"))
    want = sum(dm.dist_metric_ref(p[None], t[None], None, C, 1024) for p, t in frames)
    ref = dm.DistanceMetrics(C, 0.2).merge_(torch.from_numpy(want)).get_stats()
    assert len(k.calls) == 2 and np.array_equal(stats["F"], ref["F"]) and stats["CD_geo"] == ref["CD_geo"] > 0
    assert np.array_equal(stats["queries"], ref["queries"]) and ref["F_geo"][0] > 0.5
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "2 frames" and out[1] == "dist======" and out[2].startswith("@0.2m: F_geo=")
    more = tool.run(tool.parser().parse_args(base + ["--thresholds", "0.5", "--max-d2", "40", "--voxel-size", "0.5", "--every", "2"]),
                    device=torch.device("cpu"))
    ref = dm.DistanceMetrics(C, 0.5, (0.5,), 40).merge_(torch.from_numpy(dm.dist_metric_ref(frames[0][0][None], frames[0][1][None], None, C,
                                                                                           40))).get_stats()
    assert more["bins"] == (1,) and np.array_equal(more["F"], ref["F"]) and more["CD_sem"] == ref["CD_sem"]
    with pytest.raises(FileNotFoundError):
        tool.run(tool.parser().parse_args(["--pred", str(pred_dir), "--gt", str(tmp_path)]), device=torch.device("cpu"))


# ----------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_validate_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected

    def args():
        a = hip.EdtArgs()
        a.labels = a.target = a.mask = a.dist = a.counts = a.scratch = ptr
        a.scratch_bytes = 1 << 40
        a.batch, a.X, a.Y, a.Z = 2, 40, 24, 20
        a.label_bytes, a.target_bytes, a.n_classes, a.max_d2, a.n_slots = 1, 2, 20, 1024, 2
        a.slots[0], a.slots[1] = 0, 19
        return a

    edt, metric = hip_lib.occd_edt_sq, hip_lib.occd_dist_metric
    assert edt(None, None) == -1 and metric(None, None) == -1
    shared = (("labels", None), ("scratch", None), ("batch", 0), ("X", 0), ("Y", -2), ("Z", 0), ("label_bytes", 0), ("label_bytes", 3),
              ("label_bytes", 4), ("n_classes", 0), ("n_classes", 33), ("max_d2", 0), ("max_d2", -1), ("max_d2", 65535),
              ("scratch_bytes", 0))
    for fn, own in ((edt, (("dist", None), ("n_slots", 0), ("n_slots", 33), ("scratch_bytes", 2 * 2 * 2 * 40 * 24 * 20 - 1))),
                    (metric, (("target", None), ("counts", None), ("target_bytes", 0), ("target_bytes", 4),
                              ("scratch_bytes", 32 * 40 * 24 * 20 - 1)))):
        for field, value in shared + own:
            a = args()
            setattr(a, field, value)
            assert fn(ctypes.byref(a), None) == -1, (field, value)
        for dims in ((1 << 11, 1 << 10, 1 << 10),                           # B X Y Z past 2^31 (and the squares with it)
                     (1 << 15, 1 << 15, 1), (46341, 1, 1), (32768, 32768, 2),     # X^2 + Y^2 + Z^2 >= 2^31 on a small volume
                     (1 << 16, 1 << 16, 1 << 16)):
            a = args()
            a.batch, (a.X, a.Y, a.Z) = 1, dims
            assert fn(ctypes.byref(a), None) == -1, dims
        a = args()
        a.batch, a.X, a.Y, a.Z = 1 << 12, 1 << 10, 1 << 8, 2                # each frame is fine, the batch is not
        assert fn(ctypes.byref(a), None) == -1
    for slot in (-1, 20):
        a = args()
        a.slots[1] = slot
        assert edt(ctypes.byref(a), None) == -1
    a = args()
    a.batch, a.n_slots = 4096, 32                                            # B n_slots > 65535
    a.X, a.Y, a.Z = 8, 8, 8
    assert edt(ctypes.byref(a), None) == -1
    # additive: the ABI version did not move, the struct is what the header says
    assert hip.ABI_VERSION == 22 and {"occd_edt_sq", "occd_dist_metric"} <= set(hip.EXPORTS)
    assert ctypes.sizeof(hip.EdtArgs) == 6 * 8 + 8 + 9 * 4 + 32 * 4 + 4      # 6 pointers, one int64, 9 ints, 32 slots, tail padding
    assert (hip.EDT_MAX_CLASSES, hip.EDT_CHUNK) == (32, 8)
    assert hip.dist_metric_size(20, 1024) == 2 * 20 * 1026
    assert hip.dist_metric_scratch_bytes((256, 256, 32)) == 64 << 20 and hip.edt_scratch_bytes(2, 3, (4, 5, 6)) == 2 * 2 * 3 * 120
