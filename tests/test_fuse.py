"""CPU: temporal fusion over a sequence -- the pose reader, the grid affine, the numpy restatement `fuse_ref` of
occd_fuse_frames (float64 arithmetic on the float32-rounded coefficients; tests/test_fuse_gpu.py holds the kernel to
it), the window / reset logic of SequenceFuser and the model hook with the two kernels replaced by the restatement, and
the argument checks of both entry points before any launch."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from occdepth_amd import fuse, hip

NEAR = 2.0 ** -12          # a component of s this close to an integer may floor differently in float32 and float64
P_TOL = 5e-6               # float32 softmax against float64 (tests/test_pw_gemm.py)


# ------------------------------------------------------------------------------------------------ the restatement
def softmax64(logits):
    """(C, X, Y, Z) logits -> (S, C) float64 probabilities, voxel n = (x*Y + y)*Z + z."""
    x = np.asarray(logits, dtype=np.float64)
    x = x.reshape(x.shape[0], -1).T
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def source_coords(affine, dims):
    """s = A (i + 1/2, j + 1/2, l + 1/2) + b for every voxel, (S, 3) float64, from the float32-rounded coefficients."""
    X, Y, Z = dims
    g = np.asarray(affine, dtype=np.float32).astype(np.float64)
    i, j, l = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    c = np.stack([i, j, l], -1).reshape(-1, 3) + 0.5
    return c @ g[:9].reshape(3, 3).T + g[9:]


def fuse_ref(probs, affines, weights, dims, masks=None):
    """probs[k]: (S, C) float64 rows of source k; affines[k]: 12 coefficients; masks[k]: (S,) or None.
    -> labels (S,) uint8, n_obs (S,) uint8, prob (S, C) float64 (acc / wsum, zero rows where nothing contributed),
    near (S,) bool: a component of some source's s lies within NEAR of an integer."""
    X, Y, Z = dims
    S, C = probs[0].shape
    acc = np.zeros((S, C))
    wsum = np.zeros(S)
    n = np.zeros(S, dtype=np.int64)
    near = np.zeros(S, dtype=bool)
    for k, p in enumerate(probs):
        s = source_coords(affines[k], dims)
        near |= (np.abs(s - np.round(s)) < NEAR).any(1)
        idx = np.floor(s).astype(np.int64)
        ok = ((idx >= 0) & (idx < np.array([X, Y, Z]))).all(1)
        flat = (np.clip(idx[:, 0], 0, X - 1) * Y + np.clip(idx[:, 1], 0, Y - 1)) * Z + np.clip(idx[:, 2], 0, Z - 1)
        if masks is not None and masks[k] is not None:
            ok &= np.asarray(masks[k]).reshape(-1)[flat] != 0
        w = float(np.float32(weights[k]))
        acc[ok] += w * p[flat[ok]]
        wsum[ok] += w
        n[ok] += 1
    labels = np.where(n > 0, acc.argmax(1), 0).astype(np.uint8)          # argmax: the first maximum
    prob = np.divide(acc, wsum[:, None], out=np.zeros_like(acc), where=wsum[:, None] > 0)
    return labels, n.astype(np.uint8), prob, near


def top_two_margin(prob):
    p = np.sort(prob, 1)
    return p[:, -1] - p[:, -2]


def motion(yaw_deg, pitch_deg, shift, dims):
    """12 coefficients of a rotation (yaw about z, then pitch about y) about the grid centre plus a shift, in voxels."""
    a, b = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    R = Rz @ Ry
    c = np.asarray(dims, dtype=np.float64) / 2
    t = c - R @ c + np.asarray(shift, dtype=np.float64)
    return np.concatenate([R.reshape(9), t]).astype(np.float32)


IDENTITY = motion(0, 0, (0, 0, 0), (1, 1, 1))
GENERIC = [(7.3, 1.1, (2.37, -1.21, 0.31)), (-21.9, -2.3, (-1.63, 2.18, -0.77)), (3.1, 0.4, (5.41, 0.23, 0.12))]


# ------------------------------------------------------------------------------------------------ the pose reader
TR = "Tr: 0 -1 0 0.5 0 0 -1 0.25 1 0 0 -0.125"          # velodyne (x fwd, y left, z up) -> camera (x right, y down, z fwd)


def _write_sequence(d, poses=None, calib=None):
    os.makedirs(d, exist_ok=True)
    if poses is not None:
        with open(os.path.join(d, "poses.txt"), "w") as f:
            f.write(poses)
    if calib is not None:
        with open(os.path.join(d, "calib.txt"), "w") as f:
            f.write(calib)
    return str(d)


POSES3 = "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 2.5\n0 0 1 1 0 1 0 0 -1 0 0 4\n"


def test_read_kitti_poses_against_hand_matrices(tmp_path):
    d = _write_sequence(tmp_path / "08", POSES3, "P0: 1 0 0 0 0 1 0 0 0 0 1 0\n" + TR + "\n")
    poses = fuse.read_kitti_poses(d)
    assert sorted(poses) == [0, 1, 2] and all(p.shape == (4, 4) and p.dtype == np.float64 for p in poses.values())
    assert np.allclose(poses[0], np.eye(4), atol=1e-15)
    # frame 1: 2.5 m along the camera's z = the velodyne's x
    want = np.eye(4)
    want[0, 3] = 2.5
    assert np.allclose(poses[1], want, atol=1e-15)
    # frame 2: camera rotation about its y (down) axis by +90 deg = a velodyne yaw of -90 deg about z (up):
    # velodyne x (forward) -> -y (right).  Translation: Tr^-1 (R_cam t_Tr + t_cam) with t_Tr = (.5, .25, -.125)
    Tr = np.eye(4)
    Tr[:3] = np.array([float(w) for w in TR.split()[1:]]).reshape(3, 4)
    P = np.eye(4)
    P[:3] = np.array([0, 0, 1, 1, 0, 1, 0, 0, -1, 0, 0, 4.0]).reshape(3, 4)
    assert np.allclose(poses[2], np.linalg.inv(Tr) @ P @ Tr, atol=1e-12)
    assert np.allclose(poses[2][:3, :3], [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(poses[2][:3, :3] @ [1, 0, 0], [0, -1, 0], atol=1e-15)


@pytest.mark.parametrize("case", ["no_poses", "no_calib", "short_line", "no_tr", "short_tr", "word", "empty"])
def test_read_kitti_poses_malformed_names_the_path(tmp_path, case):
    calib = TR + "\n"
    poses = POSES3
    if case == "no_poses":
        poses = None
    elif case == "no_calib":
        calib = None
    elif case == "short_line":
        poses = "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1\n"
    elif case == "no_tr":
        calib = "P0: 1 0 0 0 0 1 0 0 0 0 1 0\n"
    elif case == "short_tr":
        calib = "Tr: 0 -1 0 0.5 0 0 -1 0.25 1 0 0\n"
    elif case == "word":
        poses = "1 0 0 0 0 1 0 0 0 0 1 x\n"
    elif case == "empty":
        poses = "\n"
    d = _write_sequence(tmp_path / "03", poses, calib)
    name = "calib.txt" if case in ("no_calib", "no_tr", "short_tr") else "poses.txt"
    with pytest.raises((OSError, ValueError), match=name) as e:
        fuse.read_kitti_poses(d)
    assert str(tmp_path / "03") in str(e.value)


# ------------------------------------------------------------------------------------------------ grid_affine
def _pose(yaw_deg, t):
    a = np.deg2rad(yaw_deg)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = t
    return T


ORIGIN = (0.0, -25.6, -2.0)


def test_grid_affine_identity_and_translation():
    p = _pose(33.0, (10.0, -4.0, 0.5))
    g = fuse.grid_affine(p, p, ORIGIN, 0.2)
    assert g.dtype == np.float32 and g.shape == (12,)
    assert np.allclose(g, IDENTITY, atol=1e-7)
    # the car moves n voxels forward between src and dst: a dst voxel lies n voxels further along x in the src grid
    for n in ((3, 0, 0), (0, -2, 0), (5, 1, -1)):
        dst = _pose(0.0, 0.2 * np.array(n, dtype=np.float64))
        g = fuse.grid_affine(_pose(0.0, (0, 0, 0)), dst, ORIGIN, 0.2)
        assert np.array_equal(g[:9], IDENTITY[:9]) and np.allclose(g[9:], n, atol=1e-6)


def test_grid_affine_composes():
    """a -> b -> c equals a -> c: (A_ab | b_ab) applied after (A_bc | b_bc), float64 composition of float64 affines."""
    a, b, c = _pose(0, (0, 0, 0)), _pose(7.0, (3.1, 0.4, 0.02)), _pose(15.5, (6.0, 1.5, -0.03))

    def f64(src, dst):                 # the same formula without the final float32 rounding
        T = np.linalg.inv(src) @ dst
        org = np.array(ORIGIN)
        return T[:3, :3], (T[:3, :3] @ org + T[:3, 3] - org) / 0.2

    for src, dst in ((a, b), (b, c), (a, c)):
        A, t = f64(src, dst)
        g = fuse.grid_affine(src, dst, ORIGIN, 0.2)
        assert np.allclose(g[:9].reshape(3, 3), A, atol=1e-7) and np.allclose(g[9:], t, rtol=1e-6, atol=1e-6)
    (Aab, tab), (Abc, tbc), (Aac, tac) = f64(a, b), f64(b, c), f64(a, c)
    # a point of c's grid -> b's grid -> a's grid
    assert np.allclose(Aab @ Abc, Aac, atol=1e-12) and np.allclose(Aab @ tbc + tab, tac, atol=1e-9)


# ------------------------------------------------------------------------------------------------ fuse_ref by hand
def test_fuse_ref_hand_case():
    dims = (3, 2, 2)
    S = 12
    p0 = np.tile([0.6, 0.4], (S, 1))
    p0[(2 * 2 + 1) * 2 + 1] = [0.5, 0.5]                 # voxel (2, 1, 1): a tie, the lowest class wins
    p1 = np.tile([0.1, 0.9], (S, 1))
    shift = IDENTITY.copy()
    shift[9] = 1.0                                       # source 1 sits one voxel further along x
    m1 = np.ones(S, dtype=np.uint8)
    m1[(1 * 2 + 0) * 2 + 0] = 0                          # source voxel (1, 0, 0) is outside source 1's mask
    labels, n_obs, prob, near = fuse_ref([p0, p1], [IDENTITY, shift], [1.0, 0.5], dims, masks=[None, m1])
    #                 x = 0: both sources, but (0, 0, 0) looks at the masked voxel; x = 1: both; x = 2: out of source 1
    want_n = np.array([[[1, 2], [2, 2]], [[2, 2], [2, 2]], [[1, 1], [1, 1]]], dtype=np.uint8)
    want_l = np.array([[[0, 1], [1, 1]], [[1, 1], [1, 1]], [[0, 0], [0, 0]]], dtype=np.uint8)   # .65 / .85 -> class 1
    assert np.array_equal(n_obs.reshape(dims), want_n) and np.array_equal(labels.reshape(dims), want_l)
    assert np.allclose(prob[1], [0.65 / 1.5, 0.85 / 1.5]) and np.allclose(prob[0], [0.6, 0.4]) and not near.any()
    # nothing contributes: label 0, n_obs 0, a zero row
    far = IDENTITY.copy()
    far[9] = 100.0
    labels, n_obs, prob, _ = fuse_ref([p1], [far], [1.0], dims)
    assert not labels.any() and not n_obs.any() and not prob.any()


# ------------------------------------------------------------------------------------------------ SequenceFuser
class KernelStandIn:
    """hip.fuse_store / hip.fuse_frames replaced by the restatement on CPU tensors; records what reaches the kernel."""

    def __init__(self):
        self.frame = None          # the frame being pushed (set by the test)
        self.stored = {}           # rows.data_ptr() -> frame
        self.calls = []

    def store(self, logits, rows):
        C = logits.shape[0]
        rows.zero_()
        rows[:, :C] = torch.from_numpy(softmax64(logits.cpu().numpy())).float()
        self.stored[rows.data_ptr()] = self.frame
        return rows

    def frames(self, rows, affines, weights, dims, n_classes, masks=None, return_prob=False):
        self.calls.append({"frames": [self.stored[r.data_ptr()] for r in rows], "weights": list(weights),
                           "affines": [np.asarray(a) for a in affines],
                           "masks": [None if m is None else m.clone() for m in masks]})
        labels, n_obs, prob, _ = fuse_ref([r[:, :n_classes].double().numpy() for r in rows], affines, weights, dims,
                                          masks=[None if m is None else m.numpy() for m in masks])
        out = torch.zeros(rows[0].shape)
        out[:, :n_classes] = torch.from_numpy(prob).float()
        return (torch.from_numpy(labels).reshape(dims), torch.from_numpy(n_obs).reshape(dims), out if return_prob else None)

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "fuse_store", self.store)
        monkeypatch.setattr(hip, "fuse_frames", self.frames)
        return self


def test_sequence_fuser_window_and_resets(monkeypatch):
    k = KernelStandIn().install(monkeypatch)
    dims, C = (4, 3, 2), 5
    S = 24
    g = torch.Generator().manual_seed(1)
    f = fuse.SequenceFuser(dims, C, ORIGIN, 0.2, window=3, decay=0.5, max_gap=5, return_prob=True)
    poses = {}

    def push(seq, frame, mask=None):
        k.frame = (seq, frame)
        poses[(seq, frame)] = _pose(2.0 * frame, (0.3 * frame, 0.01 * frame, 0.0))
        out = f.push(torch.randn((C,) + dims, generator=g), poses[(seq, frame)], key=(seq, frame), fov_mask=mask)
        assert out["y_pred"].shape == dims and out["n_obs"].shape == dims and out["ssc_prob"].shape == dims + (C,)
        assert out["y_pred"].dtype == torch.uint8 and int(out["n_obs"].min()) >= 1       # the current frame, everywhere
        return k.calls[-1]

    mask1 = torch.arange(S).reshape(dims) % 2 == 0
    assert push("A", 0)["frames"] == [("A", 0)]
    c = push("A", 1, mask1)
    assert c["frames"] == [("A", 1), ("A", 0)] and c["weights"] == [1.0, 0.5] and c["masks"] == [None, None]
    assert np.array_equal(c["affines"][0], IDENTITY)
    assert np.array_equal(c["affines"][1], fuse.grid_affine(poses[("A", 0)], poses[("A", 1)], ORIGIN, 0.2))
    c = push("A", 2)
    assert c["frames"] == [("A", 2), ("A", 1), ("A", 0)] and c["weights"] == [1.0, 0.5, 0.25]
    assert c["masks"][0] is None and c["masks"][2] is None                  # the current frame is never masked
    assert c["masks"][1].dtype == torch.uint8 and torch.equal(c["masks"][1].bool(), mask1.reshape(S))
    base = f.rows.data_ptr()
    c = push("A", 3)                                                        # the slot of frame 0 is taken over
    assert c["frames"] == [("A", 3), ("A", 2), ("A", 1)] and len(k.stored) == 3
    assert torch.equal(c["masks"][2].bool(), mask1.reshape(S)) and c["masks"][1] is None
    assert push("A", 3)["frames"] == [("A", 3)]                             # the index does not increase: reset
    assert push("A", 4)["frames"] == [("A", 4), ("A", 3)]
    assert push("B", 7)["frames"] == [("B", 7)]                             # another sequence: reset
    assert push("B", 9)["frames"] == [("B", 9), ("B", 7)]
    assert push("B", 20)["frames"] == [("B", 20)]                           # 11 > max_gap frames back: dropped
    assert push("B", 24)["frames"] == [("B", 24), ("B", 20)]
    c = push("B", 26)                                                       # 20 is 6 back, 24 only 2
    assert c["frames"] == [("B", 26), ("B", 24)] and c["weights"] == [1.0, 0.5]
    assert f.rows.data_ptr() == base and f.rows.shape == (3, S, 8) and len(k.stored) == 3     # never regrown
    with pytest.raises(ValueError):
        f.push(torch.zeros((C + 1,) + dims), np.eye(4), key=("B", 30))
    with pytest.raises(ValueError):
        fuse.SequenceFuser(dims, C, ORIGIN, 0.2, window=hip.FUSE_MAX_SOURCES + 1)


def test_sequence_fuser_equals_restatement_on_cpu(monkeypatch):
    """The labels a push returns are fuse_ref of the stored frames with the ring's weights and affines."""
    KernelStandIn().install(monkeypatch)
    dims, C = (6, 5, 3), 4
    g = torch.Generator().manual_seed(2)
    f = fuse.SequenceFuser(dims, C, ORIGIN, 0.2, window=2, decay=0.8)
    l0, l1 = (torch.randn((C,) + dims, generator=g) * 3 for _ in range(2))
    p0, p1 = _pose(0.0, (0, 0, 0)), _pose(0.0, (0.4, 0.0, 0.0))           # two voxels forward
    f.push(l0, p0, key=("00", 0))
    out = f.push(l1, p1, key=("00", 1))
    two = IDENTITY.copy()
    two[9] = 2.0
    labels, n_obs, _, _ = fuse_ref([softmax64(l1.numpy()).astype(np.float32).astype(np.float64),
                                    softmax64(l0.numpy()).astype(np.float32).astype(np.float64)],
                                   [IDENTITY, two], [1.0, 0.8], dims)
    assert np.array_equal(out["y_pred"].numpy().reshape(-1), labels)
    assert np.array_equal(out["n_obs"].numpy().reshape(-1), n_obs) and set(n_obs) == {1, 2}


# ------------------------------------------------------------------------------------------------ argument checks
def test_fuse_entry_points_validate_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected
    S = 8
    store = hip_lib.occd_fuse_store
    assert store(None, ptr, S, 20, S, 1, 20, None) == -1
    assert store(ptr, None, S, 20, S, 1, 20, None) == -1
    assert store(ptr, ptr, 0, 20, S, 1, 20, None) == -1                   # no voxel
    assert store(ptr, ptr, S, 0, S, 1, 20, None) == -1                    # C out of range
    assert store(ptr, ptr, S, 33, S, 1, 36, None) == -1
    assert store(ptr, ptr, S, 20, S, 1, 16, None) == -1                   # pitch below C
    assert store(ptr, ptr, S, 18, S, 1, 18, None) == -1                   # pitch not a multiple of 4
    assert store(ptr, ptr, S, 20, S - 1, 1, 20, None) == -1               # planes that overlap
    assert store(ptr, ptr, S, 20, 2, 3, 20, None) == -1                   # neither planes nor channels-last rows
    assert store(ptr, ptr, S, 20, 1, 16, 20, None) == -1                  # channels-last rows shorter than C

    frames = hip_lib.occd_fuse_frames
    assert frames(None, None) == -1

    def good():
        a = hip.FuseArgs()
        a.rows[0] = a.rows[1] = ptr
        a.labels = a.n_obs = ptr
        a.X, a.Y, a.Z, a.C, a.K, a.pitch = 2, 2, 2, 20, 2, 20
        return a

    for field, value in (("labels", None), ("n_obs", None), ("C", 0), ("C", 33), ("K", 0), ("K", hip.FUSE_MAX_SOURCES + 1),
                         ("X", 0), ("Y", -1), ("Z", 0), ("pitch", 19), ("pitch", 16), ("pitch", 0)):
        a = good()
        setattr(a, field, value)
        assert frames(ctypes.byref(a), None) == -1, (field, value)
    a = good()
    a.rows[1] = None                                                       # a source below K without rows
    assert frames(ctypes.byref(a), None) == -1
    a = good()
    a.X = a.Y = a.Z = 1 << 10                                              # 2^30 voxels
    assert frames(ctypes.byref(a), None) == -1
    assert hip.ABI_VERSION == 22 and ctypes.sizeof(hip.FuseArgs) == 8 * 8 * 2 + 8 * 4 + 8 * 48 + 3 * 8 + 6 * 4


# ------------------------------------------------------------------------------------------------ the model hook
def _confusion_stand_in(hist, target, logits=None, labels=None):
    pred = labels if labels is not None else logits.argmax(1)
    t, p = target.reshape(-1).long(), pred.reshape(-1).long()
    keep = t != 255
    C = hist.shape[0]
    hist += torch.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C)
    return hist


def _hook_stub(tmp_path, dataset="kitti"):
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    from occdepth_amd.models.OccDepth import OccDepth
    C = 4
    stub = SimpleNamespace(dataset=dataset, n_classes=C, full_scene_size=(8, 6, 4), project_scale=1,
                           class_names=[str(i) for i in range(C)], metrics_allreduce=False, render=None,
                           report_metrics={}, temporal_fusion=None, fused_metrics={}, logged_keys={},
                           train_metrics=SSCMetrics(C), val_metrics=SSCMetrics(C), test_metrics=SSCMetrics(C),
                           _kitti_origin=lambda batch=None: (0.0, -0.6, -2.0))
    stub._report_fov = lambda batch, target: OccDepth._report_fov(stub, batch, target)
    stub._epoch_stats = lambda metric: metric.get_stats()
    stub._print_region_report = lambda prefix: None
    stub.log = lambda key, value, **kw: stub.logged_keys.__setitem__(key, value)
    return stub


def _val_epoch(stub, steps, fused):
    from occdepth_amd.models.OccDepth import OccDepth
    for batch, logits, target in steps:
        stub.val_metrics.add_batch_logits(logits, target)                  # what step() does with the ordinary metric
        if fused:
            assert stub.temporal_fusion is not None
            OccDepth._fuse_step(stub, "val", batch, logits, target)
    hist = stub.val_metrics.hist.clone()
    OccDepth.validation_epoch_end(stub, [])
    return hist


def test_model_hook_counts_into_a_second_metric(monkeypatch, tmp_path, capsys):
    from occdepth_amd.models.OccDepth import OccDepth
    k = KernelStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    root = tmp_path / "sequences"
    _write_sequence(root / "08", "1 0 0 0 0 1 0 0 0 0 1 0\n" * 3 + "1 0 0 0 0 1 0 0 0 0 1 0.2\n" + "1 0 0 0 0 1 0 0 0 0 1 0.4\n",
                    TR + "\n")
    dims, C, S = (8, 6, 4), 4, 192
    g = torch.Generator().manual_seed(5)
    steps = []
    for frames in ((2, 3), (4,)):                                          # a two-step epoch, three frames of sequence 08
        B = len(frames)
        batch = {"sequence": ["08"] * B, "frame_id": ["%06d" % f for f in frames],
                 "fov_mask_1": [torch.rand(S, generator=g) < 0.7 for _ in frames]}
        target = torch.randint(0, C, (B,) + dims, generator=g).to(torch.uint8)
        target[:, 0, 0, 0] = 255
        steps.append((batch, torch.randn((B, C) + dims, generator=g) * 3, target))

    plain = _hook_stub(tmp_path)
    assert plain.temporal_fusion is None
    hist_plain = _val_epoch(plain, steps, fused=False)
    assert not any(key.startswith("val_fused") for key in plain.logged_keys) and plain.fused_metrics == {} and not k.calls

    stub = _hook_stub(tmp_path)
    assert OccDepth.enable_temporal_fusion(stub, str(root), window=3, decay=0.8) is stub
    k.frame = "any"
    hist = _val_epoch(stub, steps, fused=True)
    assert torch.equal(hist, hist_plain)                                   # the ordinary metric is the unfused one
    assert [c["frames"] for c in k.calls] == [["any"], ["any", "any"], ["any", "any", "any"]]
    assert k.calls[2]["weights"] == [1.0, 0.8, 0.8 ** 2]
    assert np.allclose(k.calls[2]["affines"][2][9:], [2.0, 0.0, 0.0], atol=1e-6)       # 0.4 m of 0.2 m voxels, two frames back
    assert torch.equal(k.calls[1]["masks"][1].bool(), steps[0][0]["fov_mask_1"][0])    # the earlier frame's own FOV
    assert set(stub.logged_keys) - set(plain.logged_keys) == {"val_fused/mIoU", "val_fused/IoU"}
    assert all(np.array_equal(stub.logged_keys[key], plain.logged_keys[key]) for key in plain.logged_keys)
    fm = stub.fused_metrics["val"]
    assert int(fm.hist.sum()) == 0 and sorted(stub.temporal_fusion["poses"]) == ["08"]  # reset after the epoch; poses read once
    # the test report: a second block in the same format
    stub.test_metrics.add_batch_logits(steps[0][1], steps[0][2])
    OccDepth._fuse_step(stub, "test", steps[1][0], steps[1][1], steps[1][2])
    capsys.readouterr()
    OccDepth.test_epoch_end(stub, [])
    out = capsys.readouterr().out.splitlines()
    assert out[0] == "test======" and out[5] == "test_fused======" and len(out) == 10
    assert [out[i].split("=")[0] for i in (1, 2, 4)] == [out[i].split("=")[0] for i in (6, 7, 9)]
    capsys.readouterr()
    OccDepth.test_epoch_end(plain, [])
    assert "fused" not in capsys.readouterr().out
    with pytest.raises(KeyError, match="poses.txt"):
        OccDepth._fuse_step(stub, "val", {"sequence": ["08"], "frame_id": ["000009"]}, steps[1][1], steps[1][2])


def test_enable_temporal_fusion_refusals(tmp_path):
    from occdepth_amd.models.OccDepth import OccDepth
    with pytest.raises(NotImplementedError, match="SemanticKITTI"):
        OccDepth.enable_temporal_fusion(_hook_stub(tmp_path, dataset="NYU"), str(tmp_path))
    with pytest.raises(ValueError, match="OCCDEPTH_FUSE_POSES"):
        OccDepth.enable_temporal_fusion(_hook_stub(tmp_path), "")
    with pytest.raises(ValueError):
        OccDepth.enable_temporal_fusion(_hook_stub(tmp_path), str(tmp_path), window=9)


def test_model_fusion_is_off_by_default_and_switched_by_the_environment(monkeypatch, tmp_path):
    """A constructed model: off without the variables (and occdepth_amd.fuse is not needed), on with them."""
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def model(name):
        cfg, _ = gc.occdepth_config(name)
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg)

    for var in ("OCCDEPTH_FUSE", "OCCDEPTH_FUSE_POSES", "OCCDEPTH_FUSE_DECAY"):
        monkeypatch.delenv(var, raising=False)
    m = model("kitti_flosp_small")
    assert m.temporal_fusion is None and m.fused_metrics == {}
    monkeypatch.setenv("OCCDEPTH_FUSE", "3")
    monkeypatch.setenv("OCCDEPTH_FUSE_POSES", str(tmp_path))
    monkeypatch.setenv("OCCDEPTH_FUSE_DECAY", "0.75")
    m = model("kitti_flosp_small")
    st = m.temporal_fusion
    assert (st["window"], st["decay"], st["poses_root"], st["max_gap"], st["fuser"]) == (3, 0.75, str(tmp_path), None, None)
    with pytest.raises(NotImplementedError):
        model("nyu_small")
