"""GPU: the overlap rows of occd_ccl_pair_* and PanopticMetrics (K40) against the numpy restatements of
occdepth_amd/panoptic.py, and the evaluation hook on the small synthetic model.  Rows and counters are integers and are held
with exact equality; the float64 sums of IoU within 1e-12 relative (both sides add at most a few thousand float64
quotients of the same integers, in the same order)."""
import functools

import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd import panoptic as pan
from test_ccl import HAND_SETS, STUFF, THINGS, T, hand_scene, random_volume

pytestmark = pytest.mark.gpu

SHAPES = ((2, 2 * T + 1, T + 1, T - 1), (2, 64, 48, 32))


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()   # a copy: the shared cases are read-only


def relabelled(target, seed):
    """The target with 10 % of its voxels given another label (unknown voxels get a class: a prediction has none)."""
    rng = np.random.default_rng(seed)
    pred = target.copy()
    sel = (rng.random(target.shape) < 0.1) | (target == 255)
    pred[sel] = rng.choice(np.array([0, 1, 2, 3, 9, 10], dtype=np.uint8), size=int(sel.sum()))
    return pred


def block_instances(target):
    """Instance ids that are no components: slabs of four voxels along x, per class."""
    x = np.indices(target.shape)[1]
    return (1 + x // 4 + 50 * target.astype(np.int64)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def scene(shape):
    target = random_volume(shape, 0.5, seed=sum(shape))
    pred = relabelled(target, seed=sum(shape) + 1)
    mask = np.random.default_rng(sum(shape) + 2).random(shape) < 0.7
    for a in (target, pred, mask):
        a.setflags(write=False)
    return pred, target, mask


def gpu_rows(pred, target, mask, things, stuff, connectivity, inst=None):
    p, g = _dev(pred), _dev(target)
    p_ids, p_count, p_off, _ = hip.ccl_compact(hip.ccl_segments(p, things, stuff, connectivity), p)
    g_ids, g_count, g_off, _ = hip.ccl_compact(hip.ccl_segments(g, things, stuff, connectivity, instances=_dev(inst)), g)
    return hip.ccl_overlaps(g_ids, g_count, g_off, p_ids, p_count, p_off, g, _dev(mask)).cpu().numpy(), int(g_count.sum()), int(p_count.sum())


def ref_rows(pred, target, mask, things, stuff, connectivity, inst=None):
    seg_g = pan.segments_ref(target, things, stuff, connectivity) if inst is None else pan.instance_segments_ref(target, inst, things, stuff)
    g = pan.compact_ref(seg_g, target)
    p = pan.compact_ref(pan.segments_ref(pred, things, stuff, connectivity), pred)
    return pan.overlaps_ref(g[0], g[1], p[0], p[1], target, mask)


def check_metric(pred, target, mask, things, stuff, connectivity=26, min_pred_voxels=1, inst=None, n_classes=20):
    m = pan.PanopticMetrics(n_classes, things, stuff, connectivity, min_pred_voxels)
    assert m.add_batch(_dev(pred), _dev(target), _dev(mask), _dev(inst)) is m
    counts, sums = pan.panoptic_ref(pred, target, n_classes, things, stuff, connectivity, min_pred_voxels, mask, inst)
    print("TP", counts[pan.TP].sum(), "FP", counts[pan.FP].sum(), "FN", counts[pan.FN].sum(), "sum IoU", sums[0].sum())
    assert m.counts().dtype == torch.int64 and np.array_equal(m.counts().numpy(), counts)
    assert np.allclose(m.sums().numpy(), sums, rtol=1e-12, atol=0.0)
    return m, counts, sums


def test_hand_scene_rows_and_counters():
    pred, target = hand_scene()
    rows, _, _ = gpu_rows(pred, target, None, *HAND_SETS, 26)
    want = ref_rows(pred, target, None, *HAND_SETS, 26)
    assert rows.dtype == np.int32 and np.array_equal(rows, want) and len(rows) == 11
    m, counts, _ = check_metric(pred, target, None, *HAND_SETS)
    s = m.get_stats()
    assert (counts[pan.TP, 1], counts[pan.FP, 1], counts[pan.FN, 1]) == (1, 2, 1)
    assert s["PQ_class"][1] == (3 / 5) / 2.5 and s["PQ_stuff"] == 0.4 and s["PQ_dagger"] == np.mean([(3 / 5) / 2.5, 0.8, 0.4])
    unknown, ghost = target.copy(), pred.copy()
    unknown[0, 6:9, 6, 0] = 255
    ghost[0, 6:9, 6, 0] = 1                                              # a predicted car wholly in unknown voxels counts nowhere
    void = pan.PanopticMetrics(20, *HAND_SETS).add_batch(_dev(ghost), _dev(unknown))
    assert torch.equal(void.counts(), m.counts())
    check_metric(pred, target, None, *HAND_SETS, min_pred_voxels=3)
    assert m.reset() is m and not m.counts().any() and not m.sums().any()


@pytest.mark.parametrize("instances", [False, True])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_volumes_rows_and_counters(shape, masked, instances):
    pred, target, mask = scene(shape)
    mask = mask if masked else None
    inst = block_instances(target) if instances else None
    rows, n_g, n_p = gpu_rows(pred, target, mask, THINGS, STUFF, 26, inst)
    want = ref_rows(pred, target, mask, THINGS, STUFF, 26, inst)
    print(shape, "rows", len(want), "segments", n_g, n_p)
    assert n_g.bit_length() + n_p.bit_length() <= 32                     # one sort stage
    assert rows.shape == want.shape and np.array_equal(rows, want)
    m, counts, _ = check_metric(pred, target, mask, THINGS, STUFF, inst=inst)
    assert counts[pan.TP].sum() > 0 and counts[pan.FP].sum() > 0 and counts[pan.FN].sum() > 0


def test_connectivity_6_and_min_pred_voxels():
    pred, target, mask = scene(SHAPES[0])
    check_metric(pred, target, mask, THINGS, STUFF, connectivity=6, min_pred_voxels=4)


def test_id_bits_beyond_one_word_take_the_second_sort_stage():
    """64 x 64 x 32 checkerboard under 6-connectivity: 65536 target segments, more in the prediction: 17 + 17 id bits."""
    i, j, k = np.indices((64, 64, 32))
    target = (((i + j + k) % 2) == 0).astype(np.uint8)[None]
    rng = np.random.default_rng(0)
    flip = rng.random(target.shape) < 0.1
    pred = np.where(flip, np.where(target == 1, 2, 3), target).astype(np.uint8)
    rows, n_g, n_p = gpu_rows(pred, target, None, THINGS, (), 6)
    assert n_g == 65536 and n_p > 65536 and n_g.bit_length() + n_p.bit_length() == 34
    want = ref_rows(pred, target, None, THINGS, (), 6)
    assert len(want) == n_p and np.array_equal(rows, want)
    again, _, _ = gpu_rows(pred, target, None, THINGS, (), 6)
    assert again.tobytes() == rows.tobytes()                             # two calls, identical bytes
    _, counts, _ = check_metric(pred, target, None, THINGS, (), connectivity=6)
    assert counts[pan.TP, 1] == 65536 - int((flip & (target == 1)).sum())


def test_merge_adds_counters():
    pred, target = hand_scene()
    a = pan.PanopticMetrics(20, *HAND_SETS).add_batch(_dev(pred), _dev(target))
    b = pan.PanopticMetrics(20, *HAND_SETS).add_batch(_dev(pred), _dev(target)).add_batch(_dev(target), _dev(target))
    both = pan.PanopticMetrics(20, *HAND_SETS).merge_(a).merge_(b.counts(), b.sums())
    assert torch.equal(both.counts(), a.counts() + b.counts()) and torch.equal(both.sums(), a.sums() + b.sums())
    perfect = pan.PanopticMetrics(20, *HAND_SETS).add_batch(_dev(target), _dev(target)).get_stats()
    assert perfect["PQ"] == perfect["SQ"] == perfect["RQ"] == perfect["PQ_dagger"] == 1.0


def test_tools_score_filter_and_colour(tmp_path, capsys):
    """tools/panoptic.py on a directory of pickles; --min-component / --instances of tools/render_predictions.py and
    --min-component of tools/map_sequence.py through the functions the flags call."""
    import importlib.util
    import os
    import pickle
    from types import SimpleNamespace
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")

    def load(name, alias):
        spec = importlib.util.spec_from_file_location(alias, os.path.join(tools, name))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    pred, target = hand_scene()
    for n, (p, t) in enumerate(((pred, target), (target, target))):
        with open(tmp_path / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": p[0].astype(np.uint16), "target": t[0]}, f)
    tool = load("panoptic.py", "tool_panoptic")
    args = tool.parser().parse_args(["--pred", str(tmp_path), "--gt", str(tmp_path), "--dims", "12", "12", "2"])
    stats = tool.run(args)
    counts, sums = pan.panoptic_ref(np.concatenate([pred, target]), np.concatenate([target, target]), 20, *HAND_SETS)
    want = pan.panoptic_stats(counts, sums, *HAND_SETS)
    assert stats["TP"].tolist() == want["TP"].tolist() and stats["PQ"] == pytest.approx(want["PQ"], rel=1e-12)
    out = capsys.readouterr().out
    assert "2 frames" in out and "pan======" in out

    rp = load("render_predictions.py", "tool_render_predictions")
    vol = random_volume((2, T + 3, 9, 7), 0.3, seed=8)
    vol[vol > 19] = 0
    kept, drawn = rp.component_labels(_dev(vol.astype(np.int16)), "kitti", min_component=3, instances=True)
    want = pan.filter_ref(vol, pan.KITTI_THINGS, 3)
    assert kept.dtype == torch.int16 and np.array_equal(kept.cpu().numpy(), want)
    ids = pan.compact_ref(pan.segments_ref(want, pan.KITTI_THINGS, ()), want)[0].astype(np.int64)
    colour = 1 + (((ids * 2654435761) & 0xFFFFFFFF) >> 16) % 19
    assert np.array_equal(drawn.cpu().numpy(), np.where(ids > 0, colour, want)) and (ids > 0).any()
    same, drawn_same = rp.component_labels(_dev(vol.astype(np.int16)), "kitti", min_component=3)
    assert torch.equal(same, kept) and torch.equal(drawn_same, kept)

    ms = load("map_sequence.py", "tool_map_sequence")
    seen = []

    class Map:
        n_bricks, brick_bytes = 0, 0

        def integrate(self, labels, pose, mask=None, weight=None):
            seen.append(labels.cpu().numpy())
    ms.sm = SimpleNamespace(SemanticMap=lambda *a, **k: Map())
    margs = SimpleNamespace(classes=20, voxel=0.2, origin=(0, 0, 0), dims=(12, 12, 2), max_bricks=None, load_map=None, frame_range=None,
                            every=1, fov=False, visibility=None, min_component=3, poses=str(tmp_path))
    ms.build_map(str(tmp_path), "pred", {0: np.eye(4), 1: np.eye(4)}, margs, torch.device("cuda"))
    assert np.array_equal(seen[0], pan.filter_ref(pred, pan.KITTI_THINGS, 3)[0]) and (seen[0] != pred[0]).any()
    ms.build_map(str(tmp_path), "gt", {0: np.eye(4), 1: np.eye(4)}, margs, torch.device("cuda"))
    assert np.array_equal(seen[2], target[0])                           # the target votes unfiltered


def test_model_hook_on_the_real_kernels(hip_lib, capsys):
    """enable_panoptic_metrics() on the kitti_small model the other GPU hook tests use: nothing is logged with the switch
    off, the ordinary metric is untouched with it on, and the logged values are what the restatement gives for the labels
    the hook saw."""
    from test_vox2pix_gpu import _train_setup, _without
    m, full = _train_setup()
    m = m.eval()
    batch = _without(full)
    logged = {}
    m.log = lambda key, value, **kw: logged.__setitem__(key, value)
    with torch.no_grad():
        logits = m(batch)["ssc_logit"].detach().float()
        m.validation_step(batch, 0)
        off_hist = m.val_metrics.hist.clone()
        assert m.panoptic_metrics is None
        m.validation_epoch_end([])
        assert not any("pan" in key for key in logged)
        assert m.enable_panoptic_metrics(things=(1, 2, 3), stuff=(4, 5)) is m      # classes the small model's labels carry
        m.validation_step(batch, 0)
        assert torch.equal(m.val_metrics.hist, off_hist)
        counts = m.panoptic_metrics["metrics"]["val"].counts().numpy().copy()
        sums = m.panoptic_metrics["metrics"]["val"].sums().numpy().copy()
        m.validation_epoch_end([])
        m.test_step(batch, 0)
        capsys.readouterr()
        m.test_epoch_end([])
        text = capsys.readouterr().out
    keys = {key for key in logged if key.startswith("val_pan/")}
    assert keys == {"val_pan/PQ", "val_pan/PQ_things", "val_pan/PQ_stuff", "val_pan/SQ", "val_pan/RQ", "val_pan/PQ_dagger"}
    pred = logits.argmax(1).cpu().numpy()
    target = full["target"].cpu().numpy().reshape(pred.shape)
    want_counts, want_sums = pan.panoptic_ref(pred, target, m.n_classes, (1, 2, 3), (4, 5))
    assert np.array_equal(counts, want_counts) and counts[pan.N_GT].sum() > 0 and counts[pan.N_PRED].sum() > 0
    assert np.allclose(sums, want_sums, rtol=1e-12, atol=0.0)
    ref = pan.panoptic_stats(want_counts, want_sums, (1, 2, 3), (4, 5))
    for key in keys:
        assert float(logged[key]) == pytest.approx(ref[key.split("/")[1]], rel=1e-12, abs=0.0)
    assert text.count("test_pan======") == 1 and "PQ_dagger=" in text
