"""GPU: occd_fuse_store and occd_fuse_frames against the numpy float64 restatement of tests/test_fuse.py (`fuse_ref` on
the float32-rounded coefficients, float64 softmax), and SequenceFuser on the real kernels.

Comparison rules.  float32 and float64 may floor differently only where a component of s is within evaluation error of an
integer (three float32 multiply-adds on a grid of at most 256: under 4 * 256 * 2^-24 ~ 6e-5), so voxels where any source's
s has a component within 2^-12 of an integer are left out; everywhere else n_obs is equal, the probabilities agree to
(K + 1) * 5e-6 (5e-6 per stored float32 softmax row against float64, tests/test_pw_gemm.py; a normalised weighted sum of
K such rows with weights <= 1 adds at most that per term) and the labels are equal wherever the float64 top-two margin
exceeds that bound.  Both exclusions together may cover at most 1 % of a case's voxels."""
import functools

import numpy as np
import pytest
import torch

from occdepth_amd import fuse, hip
from test_fuse import GENERIC, IDENTITY, ORIGIN, P_TOL, _pose, fuse_ref, motion, softmax64, top_two_margin

pytestmark = pytest.mark.gpu

GRID = (16, 12, 8)


def sources(dims, K):
    """K affines: the identity (the current frame), then an integer shift that pushes about 40 % of the grid out of
    bounds, a 90 degree turn about the grid centre, the three generic motions, a second shift and the identity again."""
    pool = [motion(0, 0, (3, -2, 1), dims), motion(90, 0, (0, 0, 0), dims)] + [motion(y, p, s, dims) for y, p, s in GENERIC] + \
           [motion(0, 0, (-1, 4, 0), dims), IDENTITY]
    return [IDENTITY] + pool[:K - 1]


@functools.lru_cache(maxsize=None)
def frames(dims, C, K):
    """K frames of randn * 3 logits (numpy float32, (C, X, Y, Z)), their float64 softmax rows and a 70 % mask each."""
    g = np.random.default_rng(1000 * C + 10 * K + dims[0])
    logits = [(g.standard_normal((C,) + dims) * 3).astype(np.float32) for _ in range(K)]
    masks = [(g.random(dims[0] * dims[1] * dims[2]) < 0.7).astype(np.uint8) for _ in range(K)]
    return logits, [softmax64(l) for l in logits], masks


def on_gpu(logits, layout):
    """(C, X, Y, Z) numpy -> the GPU tensor in the asked layout: contiguous planes, or a channels-last view of wider rows."""
    t = torch.from_numpy(logits).cuda()
    if layout == "planes":
        return t.contiguous()
    C = t.shape[0]
    buf = torch.full(tuple(t.shape[1:]) + (hip.round_up(C, 8),), 7.0, device="cuda")      # the pad must not be read
    buf[..., :C] = t.permute(1, 2, 3, 0)
    v = buf[..., :C].permute(3, 0, 1, 2)
    assert not v.is_contiguous() and v.stride(0) == 1
    return v


def run_case(dims, C, K, layout, masked, decay, pitch=None):
    logits, probs, masks = frames(dims, C, K)
    S = dims[0] * dims[1] * dims[2]
    pitch = hip.round_up(C, 4) if pitch is None else pitch
    rows = [hip.fuse_store(on_gpu(l, layout), torch.full((S, pitch), float("nan"), device="cuda")) for l in logits]
    aff = sources(dims, K)
    w = [decay ** k for k in range(K)]
    mk = [None] + [masks[k] if masked else None for k in range(1, K)]
    mk_gpu = [None if m is None else torch.from_numpy(m).cuda() for m in mk]
    out = hip.fuse_frames(rows, aff, w, dims, C, masks=mk_gpu, return_prob=True)
    again = hip.fuse_frames(rows, aff, w, dims, C, masks=mk_gpu, return_prob=True)
    torch.cuda.synchronize()
    labels, n_obs, prob = (t.cpu().numpy() for t in out)
    for a, b in zip(out, again):                                      # bit-identical from run to run
        assert torch.equal(a[:, :hip.round_up(C, 4)] if a.dim() == 2 else a, b[:, :hip.round_up(C, 4)] if b.dim() == 2 else b)
    ref_l, ref_n, ref_p, near = fuse_ref(probs, aff, w, dims, masks=mk)
    compare(labels.reshape(-1), n_obs.reshape(-1), prob[:, :C], ref_l, ref_n, ref_p, near, K)
    # without the probability output: the same labels
    l2, n2, none = hip.fuse_frames(rows, aff, w, dims, C, masks=mk_gpu)
    assert none is None and torch.equal(l2, out[0]) and torch.equal(n2, out[1])
    return ref_n


def compare(labels, n_obs, prob, ref_l, ref_n, ref_p, near, K):
    tol = (K + 1) * P_TOL
    keep = ~near
    sure = top_two_margin(ref_p) > tol
    print("voxels %d near-integer %d small-margin %d max |dp| %.3g n_obs %s" % (
        len(keep), int(near.sum()), int((~sure).sum()), float(np.abs(prob - ref_p)[keep].max()), np.unique(ref_n).tolist()))
    assert float((near | ~sure).mean()) <= 0.01                       # the filter cannot hide a kernel
    assert np.array_equal(n_obs[keep], ref_n[keep])
    assert float(np.abs(prob - ref_p)[keep].max()) <= tol
    assert np.array_equal(labels[keep & sure], ref_l[keep & sure])


CASES = [  # C, K, layout, masks, decay
    (20, 1, "planes", False, 1.0),
    (20, 3, "rows", True, 0.8),
    (20, 4, "planes", True, 1.0),
    (20, 4, "rows", False, 0.8),
    (20, 8, "planes", True, 0.8),
    (20, 8, "rows", False, 1.0),
    (12, 1, "rows", False, 1.0),
    (12, 3, "planes", False, 1.0),
    (12, 4, "rows", True, 0.8),
    (12, 8, "planes", True, 0.8),
]


@pytest.mark.parametrize("C,K,layout,masked,decay", CASES)
def test_fuse_frames_against_restatement(C, K, layout, masked, decay, hip_lib):
    ref_n = run_case(GRID, C, K, layout, masked, decay)
    if K == 4 and masked:
        assert set(np.unique(ref_n)) == {1, 2, 3, 4}                  # every count occurs


def test_fuse_frames_padded_pitch(hip_lib):
    run_case(GRID, 20, 3, "planes", True, 0.8, pitch=32)
    run_case(GRID, 12, 3, "rows", True, 0.8, pitch=32)


def test_fuse_frames_odd_grid(hip_lib):
    """105 voxels: the last workgroup is partly empty, for both lane-group widths."""
    run_case((5, 7, 3), 20, 4, "rows", True, 0.8)
    run_case((5, 7, 3), 12, 3, "planes", True, 1.0)


def test_fuse_frames_many_workgroups(hip_lib):
    """32 x 32 x 32: 1024 workgroups, several along every dimension."""
    run_case((32, 32, 32), 20, 4, "planes", True, 0.8)


def test_fuse_frames_nothing_contributes(hip_lib):
    """A single source that misses the grid everywhere: label 0, n_obs 0, zero rows."""
    dims, C = GRID, 20
    logits, _, _ = frames(dims, C, 1)
    S = dims[0] * dims[1] * dims[2]
    rows = hip.fuse_store(on_gpu(logits[0], "planes"), torch.empty((S, 20), device="cuda"))
    labels, n_obs, prob = hip.fuse_frames([rows], [motion(0, 0, (40, 0, 0), dims)], [1.0], dims, C, return_prob=True)
    assert not labels.any() and not n_obs.any() and not prob.any()
    nan = motion(0, 0, (0, 0, 0), dims)
    nan[9] = np.nan
    labels, n_obs, _ = hip.fuse_frames([rows], [nan], [1.0], dims, C)
    assert not labels.any() and not n_obs.any()


@pytest.mark.parametrize("layout", ["planes", "rows"])
@pytest.mark.parametrize("C,pitch", [(20, 20), (20, 32), (12, 12), (12, 32), (11, 12)])
@pytest.mark.parametrize("dims", [GRID, (5, 7, 3)])
def test_fuse_store_against_float64_softmax(dims, C, pitch, layout, hip_lib):
    g = np.random.default_rng(C + pitch)
    logits = (g.standard_normal((C,) + dims) * 3).astype(np.float32)
    S = dims[0] * dims[1] * dims[2]
    rows = torch.full((S, pitch), float("nan"), device="cuda")
    assert hip.fuse_store(on_gpu(logits, layout), rows) is rows
    got = rows.cpu().numpy()
    err = float(np.abs(got[:, :C] - softmax64(logits)).max())
    print("max |dp| %.3g" % err)
    assert err <= P_TOL
    assert not got[:, C:hip.round_up(C, 4)].any()                      # the channels the fuse pass loads beside the classes


def test_fuse_store_rows_that_are_not_16_byte_pieces(hip_lib):
    """Channels-last rows 21 floats apart: the entry point falls back to occd_softmax_channels."""
    dims, C, S = (5, 7, 3), 20, 105
    g = np.random.default_rng(21)
    wide = (g.standard_normal((S, 21)) * 3).astype(np.float32)
    src = torch.from_numpy(wide).cuda()
    rows = torch.full((S, 20), float("nan"), device="cuda")
    assert hip_lib.occd_fuse_store(src.data_ptr(), rows.data_ptr(), S, C, 1, 21, 20, torch.cuda.current_stream().cuda_stream) == 0
    ref = softmax64(wide[:, :C].T.reshape((C,) + dims))
    assert float(np.abs(rows.cpu().numpy() - ref).max()) <= P_TOL


def test_sequence_fuser_five_pushes(hip_lib):
    """window = 3, five pushes along a gentle left turn: the fourth and fifth reuse ring slots.  Every result against the
    restatement driven by the same poses, weights and masks."""
    dims, C, decay = GRID, 20, 0.8
    S = dims[0] * dims[1] * dims[2]
    origin, vs = (0.0, -1.2, -0.8), 0.2
    g = np.random.default_rng(77)
    f = fuse.SequenceFuser(dims, C, origin, vs, window=3, decay=decay, return_prob=True)
    history = []                                                       # newest first: (probs, pose, mask)
    slots = set()
    for n in range(5):
        logits = (g.standard_normal((C,) + dims) * 3).astype(np.float32)
        pose = _pose(2.3 * n, (0.43 * n, 0.05 * n * n, 0.0))
        mask = (g.random(S) < 0.7).astype(np.uint8) if n != 1 else None
        out = f.push(on_gpu(logits, "rows" if n % 2 else "planes"), pose, key=("08", 10 + n),
                     fov_mask=None if mask is None else torch.from_numpy(mask).cuda().reshape(dims).bool())
        history = [(softmax64(logits), pose, mask)] + history[:2]
        slots.add(f.entries[0]["slot"])
        K = len(history)
        aff = [IDENTITY] + [fuse.grid_affine(h[1], pose, origin, vs) for h in history[1:]]
        ref_l, ref_n, ref_p, near = fuse_ref([h[0] for h in history], aff, [decay ** k for k in range(K)], dims,
                                             masks=[None] + [h[2] for h in history[1:]])
        compare(out["y_pred"].cpu().numpy().reshape(-1), out["n_obs"].cpu().numpy().reshape(-1),
                out["ssc_prob"].cpu().numpy().reshape(S, C), ref_l, ref_n, ref_p, near, K)
    assert slots == {0, 1, 2} and [e["frame"] for e in f.entries] == [14, 13, 12]


def test_model_hook_on_the_real_kernels(hip_lib, tmp_path, capsys):
    """enable_temporal_fusion() on the kitti_small model: the ordinary metric and its printed report are untouched, and
    the second metric holds the counts of a SequenceFuser driven by hand with the same logits, poses and FOV masks."""
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    from test_fuse import TR, _write_sequence
    from test_vox2pix_gpu import _train_setup, _without
    m, full = _train_setup()
    m = m.eval()
    B = full["target"].shape[0]
    root = tmp_path / "sequences"
    _write_sequence(root / "08", "".join("1 0 0 0 0 1 0 0 0 0 1 %.1f\n" % (0.4 * n) for n in range(3 * B)), TR + "\n")
    dims = tuple(int(s) for s in m.full_scene_size)
    S = dims[0] * dims[1] * dims[2]
    g = torch.Generator().manual_seed(3)
    batches = [dict(_without(full), sequence=["08"] * B, frame_id=["%06d" % (step * B + i) for i in range(B)],
                    fov_mask_1=[(torch.rand(S, generator=g) < 0.8).cuda() for _ in range(B)]) for step in range(3)]
    with torch.no_grad():
        logits = m(batches[0])["ssc_logit"].detach().float()
        assert tuple(logits.shape[2:]) == dims
        for b in batches:
            m.test_step(b, 0)
        off_hist = m.test_metrics.hist.clone()
        assert m.temporal_fusion is None and m.fused_metrics == {}
        capsys.readouterr()
        m.test_epoch_end([])
        off_text = capsys.readouterr().out
        assert m.enable_temporal_fusion(str(root), window=3, decay=0.8) is m
        for b in batches:
            m.test_step(b, 0)
        assert torch.equal(m.test_metrics.hist, off_hist)
        fused_hist = m.fused_metrics["test"].hist.clone()
        m.test_epoch_end([])
        on_text = capsys.readouterr().out
    assert off_text.startswith("test======") and on_text.startswith(off_text)
    assert on_text[len(off_text):].startswith("test_fused======") and on_text.count("======") == 2
    poses = fuse.read_kitti_poses(str(root / "08"))
    by_hand = fuse.SequenceFuser(dims, m.n_classes, m._kitti_origin(batches[0]), 0.2, window=3, decay=0.8)
    want = SSCMetrics(m.n_classes)
    seen = set()
    for step, b in enumerate(batches):
        labels = []
        for i in range(B):
            out = by_hand.push(logits[i], poses[step * B + i], key=("08", step * B + i), fov_mask=b["fov_mask_1"][i])
            labels.append(out["y_pred"])
            seen |= set(np.unique(out["n_obs"].cpu().numpy()).tolist())
        want.add_batch(torch.stack(labels), full["target"])
    assert torch.equal(fused_hist, want.hist) and int(fused_hist.sum()) == int(off_hist.sum())
    assert seen == {1, 2, 3} and not torch.equal(fused_hist, off_hist)
    assert int(m.fused_metrics["test"].hist.sum()) == 0                              # reset with the report
