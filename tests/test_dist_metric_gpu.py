"""GPU: occd_edt_sq and occd_dist_metric (K37) against the numpy restatements of occdepth_amd/dist_metric.py
(tests/test_dist_metric.py pins those against brute force, scipy and analytic cases).  Everything is an integer: every
comparison is exact equality.

Shapes are chosen to break tiling and windows, not to resemble the workload: (2, 19, 13, 7) -- nothing a multiple of anything;
(1, 70, 9, 5) with T = 16 -- window 4, much shorter than the row; (1, 300, 3, 33) -- a row of five row tiles and z just past
a wave half; (1, 32, 32, 4) with T = 65534 -- truncation never bites, the window is the whole axis and the counters bypass
the LDS histogram (T + 2 > 4096 bins); (1, 2, 3, 30000) -- a z row too long to stage, swept in place."""
import functools

import numpy as np
import pytest
import torch

from occdepth_amd import dist_metric as dm
from occdepth_amd import hip, train_graph
from test_dist_metric import DistStandIn, counts3, random_labels

pytestmark = pytest.mark.gpu

CASES = {"odd": ((2, 19, 13, 7), 5, 1024), "short_window": ((1, 70, 9, 5), 4, 16), "long_row": ((1, 300, 3, 33), 5, 1024),
         "no_truncation": ((1, 32, 32, 4), 6, 65534), "long_z": ((1, 2, 3, 30000), 3, 16)}


def _dev(vol):
    vol = np.ascontiguousarray(vol)
    return torch.from_numpy(vol.view(np.int16) if vol.dtype == np.uint16 else vol.copy()).cuda()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> pred, target (uint8, labels >= C and 255 sprinkled in), mask (bool), C, T, and the restatement's results: the
    transform of the target for every slot, the counters without and with the mask.  Computed once, never written to."""
    shape, C, T = CASES[name]
    seed = sum(shape)
    p_occ = 0.002 if name == "long_z" else 0.08
    pred, target = random_labels(shape, C, seed, p_occ), random_labels(shape, C, seed + 1, p_occ)
    mask = np.random.default_rng(seed + 2).random(shape) < 0.7
    slots = tuple(range(C))[::-1]                                           # not in order: the list is the caller's
    out = {"pred": pred, "target": target, "mask": mask, "C": C, "T": T, "slots": slots,
           "edt": dm.edt_sq_ref(target, slots, C, T), "plain": dm.dist_metric_ref(pred, target, None, C, T),
           "masked": dm.dist_metric_ref(pred, target, mask, C, T)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def run_metric(pred, target, C, T, mask=None, counts=None):
    if counts is None:
        counts = torch.zeros(hip.dist_metric_size(C, T), dtype=torch.int64, device="cuda")
    scratch = torch.empty(hip.dist_metric_scratch_bytes(pred.shape[1:]), dtype=torch.uint8, device="cuda")
    out = hip.dist_metric(_dev(pred), _dev(target), counts, C, T, scratch, None if mask is None else torch.from_numpy(np.array(mask)).cuda())
    assert out is counts
    return counts.cpu().numpy()


# ----------------------------------------------------------------------------------------------------- occd_edt_sq
@pytest.mark.parametrize("name", sorted(CASES))
def test_edt_equals_the_restatement_on_every_value(name):
    c = case(name)
    got = _u16(hip.edt_sq(_dev(c["target"]), c["slots"], c["C"], c["T"]))
    assert got.shape == c["edt"].shape
    print(name, "max", int(got.max()), "zeros", int((got == 0).sum()), "truncated", int((got == c["T"] + 1).sum()))
    assert (got == 0).any() and got.max() > 0                               # an all-zero or all-saturated kernel cannot pass
    assert np.array_equal(got, c["edt"])


def test_edt_label_width_no_seed_every_seed_and_foreign_labels():
    shape, C, T = (1, 19, 13, 7), 5, 1024
    lab = random_labels(shape, C, 9)
    assert (lab == 255).any() and (lab == C + 1).any()                      # labels >= C are in it and are no seeds
    want = dm.edt_sq_ref(lab, range(C), C, T)
    wide = lab.astype(np.uint16)
    free = np.argwhere(wide == 0)
    for n, idx in enumerate(free[::37]):
        wide[tuple(idx)] = (258, 300, 65535, 511, 257)[n % 5]               # the low byte is a class; the label is not
    assert np.array_equal(_u16(hip.edt_sq(_dev(wide), range(C), C, T)), want)
    assert np.array_equal(want, dm.edt_sq_ref(wide, range(C), C, T))
    empty = np.zeros(shape, dtype=np.uint8)
    empty[0, 3, 3, 3], empty[0, 10, 2, 1] = 255, C                          # nothing that is a seed
    assert (_u16(hip.edt_sq(_dev(empty), [0, 1, 4], C, T)) == T + 1).all()
    full = np.full(shape, 3, dtype=np.uint8)
    got = _u16(hip.edt_sq(_dev(full), [0, 3, 2], C, T))
    assert not got[:, :2].any() and (got[:, 2] == T + 1).all()
    # reusable buffers: the same values, written where the caller said
    out = torch.empty((1, C) + shape[1:], dtype=torch.int16, device="cuda")
    scratch = torch.empty(hip.edt_scratch_bytes(1, C, shape[1:]), dtype=torch.uint8, device="cuda")
    assert hip.edt_sq(_dev(lab), range(C), C, T, out=out, scratch=scratch) is out and np.array_equal(_u16(out), want)
    with pytest.raises(RuntimeError, match="scratch"):
        hip.edt_sq(_dev(lab), range(C), C, T, scratch=scratch[:-1])


# ----------------------------------------------------------------------------------------------------- occd_dist_metric
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_counter_equals_the_restatement(name):
    c = case(name)
    C, T = c["C"], c["T"]
    got = run_metric(c["pred"], c["target"], C, T)
    g3 = counts3(got, C, T)
    print(name, "queries", g3.sum(2).tolist(), "bin 0", g3[:, :, 0].tolist(), "overflow", g3[:, :, T + 1].tolist())
    assert (c["target"] == 255).any() and g3[:, 0].sum() > 0                # an all-zero kernel cannot pass
    assert np.array_equal(got, c["plain"])
    masked = run_metric(c["pred"], c["target"], C, T, mask=c["mask"])
    assert np.array_equal(masked, c["masked"]) and masked.sum() < got.sum()
    # 16-bit predictions (with labels past a byte that are no class) and 16-bit targets
    wide = c["pred"].astype(np.uint16)
    wide[wide == C + 1] = 256 + 1
    assert np.array_equal(run_metric(wide, c["target"], C, T), c["plain"])
    assert np.array_equal(run_metric(c["pred"], c["target"].astype(np.uint16), C, T, mask=c["mask"].astype(np.uint8)), c["masked"])


def test_zero_mask_accumulation_and_batches():
    c = case("odd")
    C, T = c["C"], c["T"]
    counts = torch.arange(hip.dist_metric_size(C, T), dtype=torch.int64, device="cuda")
    before = counts.cpu().numpy().copy()
    assert np.array_equal(run_metric(c["pred"], c["target"], C, T, mask=np.zeros_like(c["mask"]), counts=counts), before)   # untouched
    run_metric(c["pred"], c["target"], C, T, counts=counts)
    twice = run_metric(c["pred"], c["target"], C, T, mask=c["mask"], counts=counts)
    assert np.array_equal(twice, before + c["plain"] + c["masked"])         # added to, never zeroed
    # B = 3 against the sum of three B = 1 calls
    shape = (3, 19, 13, 7)
    pred, target = random_labels(shape, C, 41), random_labels(shape, C, 42)
    mask = np.random.default_rng(43).random(shape) < 0.5
    together = run_metric(pred, target, C, T, mask=mask)
    apart = sum(run_metric(pred[b:b + 1], target[b:b + 1], C, T, mask=mask[b:b + 1]) for b in range(3))
    assert np.array_equal(together, apart) and together.any()
    assert np.array_equal(together, dm.dist_metric_ref(pred, target, mask, C, T))


@pytest.mark.parametrize("name", ["odd", "no_truncation"])
def test_the_fused_count_agrees_with_edt_then_counting(name):
    """The two entry points agree with each other, not only with the restatement."""
    c = case(name)
    C, T = c["C"], c["T"]
    pred, target, mask = c["pred"], c["target"], c["mask"]
    Dt = _u16(hip.edt_sq(_dev(target), range(C), C, T))
    Dp = _u16(hip.edt_sq(_dev(pred), range(C), C, T))
    query = (target != 255) & mask
    want = np.zeros((2, C, T + 2), dtype=np.int64)
    for s in range(C):
        want[0, s] = np.bincount(Dt[:, s][query & dm.seeds_of(pred, s, C)], minlength=T + 2)
        want[1, s] = np.bincount(Dp[:, s][query & dm.seeds_of(target, s, C)], minlength=T + 2)
    assert np.array_equal(run_metric(pred, target, C, T, mask=mask), want.reshape(-1))


# ----------------------------------------------------------------------------------------------------- DistanceMetrics
def test_distance_metrics_on_the_gpu_equals_the_stand_in_path(monkeypatch):
    c = case("odd")
    C, T = c["C"], c["T"]

    def feed(device):
        m = dm.DistanceMetrics(C, 0.2, max_d2=T)
        m.add_batch(torch.from_numpy(c["pred"].copy()).to(device), torch.from_numpy(c["target"].copy()).to(device))
        m.add_batch(torch.from_numpy(c["pred"].astype(np.int64)).to(device), torch.from_numpy(c["target"].astype(np.int32)).to(device),
                    torch.from_numpy(c["mask"].copy()).to(device))
        return m

    on_gpu = feed("cuda")
    assert on_gpu.counts().is_cuda and on_gpu.scratch_bytes() == 32 * 19 * 13 * 7
    assert np.array_equal(on_gpu.counts().cpu().numpy(), c["plain"] + c["masked"])
    DistStandIn().install(monkeypatch)
    stand_in = feed("cpu")
    assert torch.equal(on_gpu.counts().cpu(), stand_in.counts())
    a, b = on_gpu.get_stats(), stand_in.get_stats()
    assert np.array_equal(a["F"], b["F"]) and a["CD_geo"] == b["CD_geo"] > 0.0 and 0.0 < a["F_geo"][0] < 1.0


def test_capture_and_replay():
    """Captured on one stream (no parallel branches): two replays add twice what one eager call adds."""
    c = case("odd")
    C, T = c["C"], c["T"]
    m = dm.DistanceMetrics(C, 0.2, max_d2=T)
    p, t, k = _dev(c["pred"]), _dev(c["target"]), torch.from_numpy(c["mask"].copy()).cuda()
    m.add_batch(p, t, k)                                                    # eager: allocates the counters and the scratch
    eager = m.counts().clone()
    assert np.array_equal(eager.cpu().numpy(), c["masked"])
    m.reset()
    torch.cuda.synchronize()
    g = train_graph.new_graph()
    with torch.cuda.graph(g):
        m.add_batch(p, t, k)
    train_graph.seal_graph(g)
    torch.cuda.synchronize()
    assert not m.counts().any()                                             # capturing ran nothing
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.counts(), 2 * eager)


def test_model_hook_on_the_real_kernels(hip_lib, capsys):
    """enable_distance_metrics() on the kitti_small model the other GPU hook tests use (its logits are (64, 64, 16)): the
    ordinary metric is untouched, the logged keys are finite and are what the restatement gives for the same labels."""
    from test_vox2pix_gpu import _train_setup, _without
    m, full = _train_setup()
    m = m.eval()
    batch = _without(full)
    logged = {}
    m.log = lambda key, value, **kw: logged.__setitem__(key, value)
    with torch.no_grad():
        logits = m(batch)["ssc_logit"].detach().float()
        dims = tuple(int(d) for d in logits.shape[2:])
        assert dims == (64, 64, 16)
        m.validation_step(batch, 0)
        off_hist = m.val_metrics.hist.clone()
        assert m.dist_metrics is None
        m.validation_epoch_end([])
        assert not any("dist" in key for key in logged)
        assert m.enable_distance_metrics() is m
        m.validation_step(batch, 0)
        assert torch.equal(m.val_metrics.hist, off_hist)
        counts = m.dist_metrics["metrics"]["val"].counts().cpu().numpy().copy()
        m.validation_epoch_end([])
        m.test_step(batch, 0)
        capsys.readouterr()
        m.test_epoch_end([])
        text = capsys.readouterr().out
    keys = {key for key in logged if key.startswith("val_dist/")}
    assert keys == {"val_dist/F_geo@0.2", "val_dist/F_geo@0.4", "val_dist/F_geo@0.8", "val_dist/F_sem@0.2", "val_dist/F_sem@0.4",
                    "val_dist/F_sem@0.8", "val_dist/CD_geo", "val_dist/CD_sem"}
    assert all(np.isfinite(float(logged[key])) for key in keys)
    B = logits.shape[0]
    pred = logits.argmax(1).cpu().numpy()
    target = full["target"].cpu().numpy().reshape(pred.shape)
    assert np.array_equal(counts, dm.dist_metric_ref(pred, target, None, m.n_classes, 1024)) and counts.any()
    ref = dm.DistanceMetrics(m.n_classes, 0.2 * float(m.full_scene_size[0]) / dims[0]).merge_(torch.from_numpy(counts)).get_stats()
    assert float(logged["val_dist/CD_geo"]) == ref["CD_geo"] and float(logged["val_dist/F_geo@0.4"]) == ref["F_geo"][1]
    assert text.count("test_dist======") == 1 and "CD_geo=" in text and B >= 1
