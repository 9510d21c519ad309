"""occd_kitti_labels on the GPU (targets.kitti_labels) against tests/golden/kitti_raw_labels.npz -- the reference's own
readers, remap table, masking and _downsample_label on synthetic raw SemanticKITTI voxel files -- bit for bit; the step and
the captured training step on a batch that carries the raw files instead of `target`; tools/preprocess_kitti_gpu.py."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_kitti_labels import CASES, ROOT, gold

pytestmark = pytest.mark.gpu


def _case(name):
    g = gold()
    frames, scene = CASES[name]
    return g, frames, scene, tuple(g[f"{name}.{k}"] for k in ("raw", "invalid_bits", "occluded_bits"))


def _offset_rows(rows, dtype):
    """`rows` (B, n) on the GPU as a view that starts one element into its storage: for 16-bit labels the data pointer is
    2-byte aligned and no more."""
    flat = np.concatenate([np.zeros(1, dtype=rows.dtype), rows.reshape(-1)])
    t = torch.from_numpy(flat).cuda()[1:].view(rows.shape)
    assert t.storage_offset() == 1 and t.is_contiguous()
    return t if dtype is None else t.view(dtype)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kitti_labels_bit_exact_gpu(hip_lib, name):
    from occdepth_amd import targets
    g, frames, scene, (raw, inv, occ) = _case(name)
    want = g[f"{name}.target_1_1"]
    want_occ = g[f"{name}.occluded"]
    inv_d, occ_d = torch.from_numpy(inv).cuda(), torch.from_numpy(occ).cuda()
    variants = {"uint16": torch.from_numpy(raw).cuda(), "int16": torch.from_numpy(raw).cuda().view(torch.int16),
                "uint16+2B": _offset_rows(raw, None), "int16+2B": _offset_rows(raw, torch.int16)}
    assert variants["uint16"].data_ptr() % 16 == 0 and variants["uint16+2B"].data_ptr() % 16 == 2
    for tag, r in variants.items():
        target = targets.kitti_labels(r, inv_d, scene_size=scene)
        assert target.dtype == torch.uint8 and tuple(target.shape) == (frames,) + scene, tag
        assert np.array_equal(target.cpu().numpy().astype(np.float32), want), tag
        target, occluded = targets.kitti_labels(r, inv_d, occ_d, scene_size=scene, check=True)
        assert occluded.dtype == torch.uint8 and tuple(occluded.shape) == (frames,) + scene, tag
        assert np.array_equal(target.cpu().numpy().astype(np.float32), want), tag
        assert np.array_equal(occluded.cpu().numpy(), want_occ), tag
    # masks one byte into their storage, per-sample lists, an explicit table
    target, occluded = targets.kitti_labels(list(variants["uint16"]), _offset_rows(inv, None), _offset_rows(occ, None),
                                            scene_size=scene, lut=torch.from_numpy(targets.kitti_remap_lut()))
    assert np.array_equal(target.cpu().numpy().astype(np.float32), want)
    assert np.array_equal(occluded.cpu().numpy(), want_occ)
    # the 1:8 labels of the reference's preprocessing
    coarse = targets.downsample_label(target, 8)
    assert coarse.dtype == torch.uint8 and np.array_equal(coarse.cpu().numpy(), g[f"{name}.target_1_8"])


def test_kitti_labels_counts_out_of_range_gpu(hip_lib):
    from occdepth_amd import targets
    g, frames, scene, (raw, inv, occ) = _case("g32b2")
    n = raw.shape[1]
    want = g["g32b2.target_1_1"].reshape(frames, n)
    inv_d = torch.from_numpy(inv).cuda()
    clean = torch.from_numpy(raw).cuda()
    planted_np = raw.copy()
    spots = [(0, 0), (0, n // 2 + 3), (frames - 1, n - 1)]                  # first voxel, one in the middle, last voxel
    for (b, i), value in zip(spots, (359, 1000, 65535)):
        planted_np[b, i] = value
    planted = torch.from_numpy(planted_np).cuda()

    def run(r):
        target, _, count = targets.kitti_labels_counted(r, inv_d, scene_size=scene)
        return target.reshape(frames, n).cpu().numpy(), int(count.item())

    before, c0 = run(clean)
    got, c1 = run(planted)
    got16, c16 = run(planted.view(torch.int16))
    after, c2 = run(clean)
    assert (c0, c1, c16, c2) == (0, 3, 3, 0)                                # the kernel sets its counter on every launch
    assert np.array_equal(before.astype(np.float32), want) and np.array_equal(after.astype(np.float32), want)
    expect = want.copy()
    for b, i in spots:
        expect[b, i] = 255
    assert np.array_equal(got.astype(np.float32), expect) and np.array_equal(got16, got)
    with pytest.raises(IndexError, match="3 raw label"):
        targets.kitti_labels(planted, inv_d, scene_size=scene, check=True)
    assert targets.kitti_labels(planted, inv_d, scene_size=scene).shape == (frames,) + scene      # unchecked: no raise


def test_kitti_labels_rejects_bad_arguments_gpu(hip_lib):
    from occdepth_amd import targets
    raw = torch.zeros((1, 64), dtype=torch.uint16, device="cuda")
    inv = torch.zeros((1, 8), dtype=torch.uint8, device="cuda")
    assert int(targets.kitti_labels(raw, inv, scene_size=(4, 4, 4)).sum()) == 0
    with pytest.raises(RuntimeError, match="raw must be"):                     # N of the grid, not of the tensor
        targets.kitti_labels(raw, inv, scene_size=(4, 4, 8))
    with pytest.raises(RuntimeError, match="invalid_bits"):                    # mask lengths
        targets.kitti_labels(raw, inv[:, :7], scene_size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="occluded_bits"):
        targets.kitti_labels(raw, inv, inv[:, :4], scene_size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="uint16"):                          # dtypes
        targets.kitti_labels(raw.view(torch.int16).to(torch.int32), inv, scene_size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="uint8"):
        targets.kitti_labels(raw, inv.to(torch.int32), scene_size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="lut"):
        targets.kitti_labels(raw, inv, scene_size=(4, 4, 4), lut=np.zeros(4, dtype=np.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        targets.kitti_labels(raw.cpu(), inv, scene_size=(4, 4, 4))


# ------------------------------------------------------------------------------------------------ the model
def _raw_frame(target):
    """Raw files whose decode is `target` (X, Y, Z) uint8 numpy: classes through the inverse label map, 255 as an invalid
    bit over an arbitrary label.  -> (raw (N,) uint16, invalid_bits (N / 8,) uint8)."""
    from occdepth_amd.output import KITTI_LEARNING_MAP_INV
    flat = target.reshape(-1)
    inverse = np.asarray(KITTI_LEARNING_MAP_INV, dtype=np.uint16)
    raw = np.where(flat == 255, np.uint16(40), inverse[np.minimum(flat, 19)]).astype(np.uint16)
    return raw, np.packbits(flat == 255)


def _frames():
    """kitti_small model, its batch without any target, and three frames (target, raw, invalid_bits) on the GPU: the
    "mixed" target of the train_targets fixture, rolled along x."""
    from test_train_targets import TARGET_KEYS, _small_batch
    m, full = _small_batch()
    base = {k: v for k, v in full.items() if k not in TARGET_KEYS and k != "target"}
    frames = []
    for shift in (0, 8, 24):
        t = np.roll(full["target"][0].cpu().numpy(), shift, axis=0)
        raw, inv = _raw_frame(t)
        frames.append((torch.from_numpy(t)[None].cuda(), torch.from_numpy(raw)[None].cuda(),
                       torch.from_numpy(inv)[None].cuda()))
    return m, base, frames


def test_step_decodes_raw_labels_gpu(hip_lib):
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    m, base, frames = _frames()
    m = m.eval()
    assert m.gpu_targets == "auto" and m.fp_loss and m.context_prior and m.relation_loss
    for target, raw, inv in frames[:2]:
        batches = {"target": dict(base, target=target),
                   "raw": dict(base, voxel_label_raw=raw, voxel_invalid_bits=inv),
                   "raw int16": dict(base, voxel_label_raw=raw.view(torch.int16), voxel_invalid_bits=inv, target=[])}
        logged = {}
        for name, batch in batches.items():
            for step_type in ("train", "val", "test"):
                m.cur_batch = 3
                with torch.no_grad():
                    m.step(batch, step_type, SSCMetrics(m.n_classes, device="cuda") if step_type == "train" else None)
                logged[name, step_type] = {k: float(v) for k, v in m.logged.items()}
            if name != "target":
                decoded, occluded = m._step_labels(batch, "cuda")
                assert occluded is None and torch.equal(decoded, target)            # the decoded target, bit for bit
                assert "target" not in batch or batch["target"] == []
        print(logged)
        for name in ("raw", "raw int16"):
            for step_type in ("train", "val", "test"):
                ref, got = logged["target", step_type], logged[name, step_type]
                assert sorted(ref) == sorted(got) and all(np.isfinite(v) for v in ref.values())
                for k in ref:
                    assert got[k] == pytest.approx(ref[k], rel=1e-6, abs=1e-12), (name, step_type, k)
    m.gpu_targets = False
    with pytest.raises(RuntimeError, match="OCCDEPTH_GPU_TARGETS"):
        with torch.no_grad():
            m.step(batches["raw"], "train", None)


def test_whole_step_hipgraph_decodes_raw_labels_gpu(hip_lib):
    """GraphedTrainStep on a batch that carries the raw files captures the decode with the step; three replays, each with
    another frame copied in, match the same captured step fed the decoded `target` (the bounds of
    test_train_targets.test_whole_step_hipgraph_builds_targets_gpu)."""
    from occdepth_amd import train_graph
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, base, frames = _frames()
    assert not torch.equal(frames[0][0], frames[1][0]) and not torch.equal(frames[1][0], frames[2][0])
    runs = {}
    for mode in ("target", "raw"):
        def batch_of(frame):
            target, raw, inv = frame
            if mode == "target":
                return dict(base, target=target.clone())
            return dict(base, voxel_label_raw=raw.view(torch.int16).clone(), voxel_invalid_bits=inv.clone())
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        opt = train_graph.make_capturable(torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True))
        gs = train_graph.GraphedTrainStep(m, opt, batch_of(frames[0]), warmup=2)
        assert gs.capture(), gs.error
        losses = []
        for frame in frames:
            gs.load_batch(batch_of(frame))
            losses.append(float(gs()))
            if mode == "raw":
                assert "target" not in gs.batch
                assert torch.equal(m._step_labels(gs.batch, "cuda")[0], frame[0])   # what the replay decoded
        terms = {k: float(v) for k, v in m.logged.items()}
        runs[mode] = (losses, terms, next(iter(m.net_3d_decoder.parameters())).detach().float().cpu().clone())
    (lt, tt, pt), (lr, tr, pr) = runs["target"], runs["raw"]
    print("target", lt, "raw", lr)
    assert any(k.endswith("loss_frustums") for k in tr) and sorted(tt) == sorted(tr)
    assert abs(lt[0] - lr[0]) <= 1e-5 * abs(lt[0]), (lt, lr)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(lt, lr)), (lt, lr)
    assert float((pt - pr).abs().max() / pt.abs().max()) < 5e-3


# ------------------------------------------------------------------------------------------------ the tool
def test_preprocess_tool_writes_reference_files_gpu(hip_lib, tmp_path):
    spec = importlib.util.spec_from_file_location("preprocess_kitti_gpu",
                                                  os.path.join(ROOT, "tools", "preprocess_kitti_gpu.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g, frames, scene, (raw, inv, occ) = _case("g32b2")
    voxels, out = tmp_path / "voxels", tmp_path / "labels" / "00"
    voxels.mkdir()
    for f in range(frames):
        raw[f].tofile(voxels / ("%06d.label" % f))
        inv[f].tofile(voxels / ("%06d.invalid" % f))
    written = tool.preprocess_sequence(str(voxels), str(out), scene_size=scene, batch=8)
    assert sorted(os.path.basename(p) for p in written) == sorted("%06d_%s.npy" % (f, s) for f in range(frames)
                                                                  for s in ("1_1", "1_8"))
    for f in range(frames):
        full, coarse = np.load(out / ("%06d_1_1.npy" % f)), np.load(out / ("%06d_1_8.npy" % f))
        for got, want in ((full, g["g32b2.target_1_1"][f]), (coarse, g["g32b2.target_1_8"][f])):
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    stamps = {p: os.stat(p).st_mtime_ns for p in written}
    assert tool.preprocess_sequence(str(voxels), str(out), scene_size=scene, batch=8) == []       # nothing to do
    os.remove(out / "000001_1_8.npy")                                                              # one file missing
    again = tool.preprocess_sequence(str(voxels), str(out), scene_size=scene, batch=1)
    assert [os.path.basename(p) for p in again] == ["000001_1_8.npy"]
    assert np.array_equal(np.load(again[0]), g["g32b2.target_1_8"][1])
    assert all(os.stat(p).st_mtime_ns == s for p, s in stamps.items() if p != again[0])
