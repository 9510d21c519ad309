"""CPU: the sequence-level semantic map (K30) -- `MapRef`, the numpy restatement of occd_map_integrate and of the
extraction (a dict world voxel -> int64 vote vector, driven by the same int64 fixed-point arithmetic;
tests/test_map_gpu.py holds the kernels to it with exact equality), the quantised coefficients, the brick selection, the
directory and pool of SemanticMap with the kernels replaced by a stand-in built on the restatement, map_confusion, the
PLY writer, the model hook, and the argument checks of the four entry points before any launch."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd import semantic_map as sm

V = 0.2
B = 16
GRIDS = {(40, 24, 20): (-3.1, -2.3, -1.7), (16, 12, 8): (-1.5, -1.1, -0.7)}    # dims -> origin (m): the grid straddles zero
LOCAL = np.stack(np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
POS_TOL = 46 * 2.0 ** -17          # (3 * 15 + 1) half-ulps of the 16 fractional bits


def pose(yaw_deg=0.0, pitch_deg=0.0, t=(0.0, 0.0, 0.0)):
    a, b = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    P = np.eye(4)
    P[:3, :3] = Rz @ Ry
    P[:3, 3] = t
    return P


def yaw90(t=(0.0, 0.0, 0.0)):
    P = np.eye(4)
    P[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]          # exact, unlike cos(pi / 2)
    P[:3, 3] = t
    return P


def sequence(dims):
    """Identity, an integer shift, a 90 degree yaw, two generic yaw + pitch motions, a jump of more than a grid length."""
    return [pose(), pose(t=(0.4, -0.2, 0.2)), yaw90((0.2, 0.4, 0.0)), pose(17.3, 2.1, (1.13, -0.57, 0.21)),
            pose(-31.7, -3.4, (-0.71, 0.93, -0.33)), pose(5.2, 0.7, (dims[0] * V * 1.5 + 0.37, 0.3, 0.1))]


# ------------------------------------------------------------------------------------------------ the restatement
def ref_coefficients(P, keys, origin, v=V):
    """Aq (3, 3), cq (n, 3) as int64: rint(R^T 2^16), rint(c_k 2^16), c_k = (R^T ((16 k + 1/2) v - t) - o) / v."""
    R, t = P[:3, :3], P[:3, 3]
    c = (((B * np.asarray(keys, dtype=np.float64) + 0.5) * v - t) @ R - np.asarray(origin, dtype=np.float64)) / v
    return np.rint(R.T * 65536.0).astype(np.int64), np.rint(c * 65536.0).astype(np.int64), c


def fixed_index(Aq, cq):
    """(3, 3), (n, 3) int64 -> the frame index (n, 4096, 3) of every brick-local voxel: (Aq (i, j, l) + cq) >> 16."""
    gq = LOCAL[None] @ Aq.T[None] + cq[:, None, :]
    assert np.abs(gq).max() < 2 ** 31
    return gq >> 16


def voting_labels(idx, labels, mask, dims, C):
    """idx (n, 4096, 3) -> (n, 4096) int64: the label that voxel votes for, -1 where it does not vote."""
    X, Y, Z = dims
    ok = ((idx >= 0) & (idx < np.array([X, Y, Z]))).all(-1)
    flat = (np.clip(idx[..., 0], 0, X - 1) * Y + np.clip(idx[..., 1], 0, Y - 1)) * Z + np.clip(idx[..., 2], 0, Z - 1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)[flat]
    if mask is not None:
        ok &= np.asarray(mask).reshape(-1)[flat] != 0
    return np.where(ok & (lab < C), lab, -1)


def generous_bricks(P, origin, dims, v=V, margin=1):
    """Every brick of the range of the grid's corners in world voxels, `margin` bricks wider on every side."""
    corners = np.array([[x, y, z] for x in (0, dims[0]) for y in (0, dims[1]) for z in (0, dims[2])], dtype=np.float64)
    world = ((corners * v + np.asarray(origin)) @ P[:3, :3].T + P[:3, 3]) / v
    lo = np.floor(world.min(0) / B).astype(np.int64) - margin
    hi = np.floor(world.max(0) / B).astype(np.int64) + margin
    k = np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in range(3)), indexing="ij")
    return np.stack(k, -1).reshape(-1, 3)


class MapRef:
    """world voxel (I, J, L) -> int64 vote vector; knows nothing of bricks but the 16-voxel period of the coefficients."""

    def __init__(self, n_classes, origin, dims, v=V):
        self.C, self.origin, self.dims, self.v = n_classes, origin, dims, v
        self.votes = {}
        self._bricks = None

    def integrate(self, labels, P, mask=None):
        self._bricks = None
        keys = generous_bricks(P, self.origin, self.dims, self.v)
        Aq, cq, _ = ref_coefficients(P, keys, self.origin, self.v)
        lab = voting_labels(fixed_index(Aq, cq), labels, mask, self.dims, self.C)
        n, vox = np.nonzero(lab >= 0)
        world = B * keys[n] + LOCAL[vox]
        for w, c in zip(map(tuple, world.tolist()), lab[n, vox].tolist()):
            self.votes.setdefault(w, np.zeros(self.C, dtype=np.int64))[c] += 1
        return self

    def bricks(self):
        """{key: (16, 16, 16, C)} of every brick with a vote (one pass over the voxels, kept until the next frame)."""
        if self._bricks is None:
            out = {}
            for w, vec in self.votes.items():
                key = tuple(c // B for c in w)
                out.setdefault(key, np.zeros((B, B, B, self.C), dtype=np.int64))[tuple(c % B for c in w)] = vec
            self._bricks = out
        return self._bricks

    def brick(self, key):
        """(16, 16, 16, C) int64 votes of one brick."""
        return self.bricks().get(tuple(int(c) for c in key), np.zeros((B, B, B, self.C), dtype=np.int64))

    def labels(self, key):
        """(16, 16, 16) uint8: argmax (np.argmax: the lowest class on a tie), 255 without a vote."""
        v = self.brick(key)
        return np.where(v.sum(-1) > 0, v.argmax(-1), 255).astype(np.uint8)

    def extract(self, min_obs=1, include_empty=False):
        """coords (N, 3) int32, labels (N,) uint8, n_obs (N,) uint16 in the order of the contract: bricks by ascending
        key, voxels in (i, j, l) order -- which is the ascending order of (key, local) tuples."""
        rows = []
        for w, vec in self.votes.items():
            n, lab = int(vec.sum()), int(vec.argmax())
            if n >= max(min_obs, 1) and (include_empty or lab != 0):
                rows.append((tuple(c // B for c in w) + tuple(c % B for c in w), w, lab, min(n, 65535)))
        rows.sort()
        return (np.array([r[1] for r in rows], dtype=np.int32).reshape(-1, 3), np.array([r[2] for r in rows], dtype=np.uint8),
                np.array([r[3] for r in rows], dtype=np.uint16))


def confusion_ref(pred, gt, C):
    """[target, prediction] counts over the world voxels both restatements observed."""
    hist = np.zeros((C, C), dtype=np.int64)
    for w, g in gt.votes.items():
        p = pred.votes.get(w)
        if p is not None and p.sum() > 0 and g.sum() > 0:
            hist[int(g.argmax()), int(p.argmax())] += 1
    return hist


def frames_for(dims, C, seed, n, label_bytes=1, masked=False):
    """n frames of labels (with 255 and one label >= C in them) and masks (70 % set, or None)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        lab = rng.integers(0, C, dims).astype(np.uint8 if label_bytes == 1 else np.uint16)
        lab[rng.random(dims) < 0.1] = 255
        lab[tuple(d // 2 for d in dims)] = C                      # a label past the classes that is not 255
        if label_bytes == 2:
            lab[1, 1, 1] = 300                                       # and one that does not fit a byte
        out.append((lab, (rng.random(dims) < 0.7) if masked else None))
    return out


# ------------------------------------------------------------------------------------------------ the kernel stand-in
class KernelStandIn:
    """hip.map_integrate / map_brick_labels / map_extract on CPU tensors, from the tables the host side builds."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "map_integrate", self.integrate)
        monkeypatch.setattr(hip, "map_brick_labels", self.brick_labels)
        monkeypatch.setattr(hip, "map_extract", self.extract)
        return self

    @staticmethod
    def _u16(votes):
        assert votes.dtype == torch.int16 and votes.dim() == 3 and votes.shape[1] == B ** 3 and votes.is_contiguous()
        return votes.numpy().view(np.uint16)                          # shares the tensor's memory

    def integrate(self, votes, table, labels, dims, n_classes, mask=None, table_host=None):
        v, t = self._u16(votes), table.numpy().astype(np.int64)
        assert t.shape[1] == 16 and len(set(t[:, 0].tolist())) == len(t) and t[:, 0].min() >= 0 and t[:, 0].max() < len(v)
        assert table_host is not None and torch.equal(table_host, table)
        self.calls.append({"n": len(t), "mask": mask is not None, "dtype": labels.dtype})
        lab = labels.numpy().reshape(-1)
        lab = lab.view(np.uint16) if lab.dtype == np.int16 else lab
        m = None if mask is None else mask.numpy().reshape(-1)
        for row in t:
            vote = voting_labels(fixed_index(row[4:13].reshape(3, 3), row[None, 13:16]), lab, m, dims, n_classes)[0]
            vox = np.nonzero(vote >= 0)[0]
            cur = v[row[0], vox, vote[vox]].astype(np.int64)
            v[row[0], vox, vote[vox]] = np.minimum(cur + 1, 65535).astype(np.uint16)
        return votes

    def _decide(self, votes, table, n_classes):
        v, t = self._u16(votes), table.numpy().astype(np.int64)
        assert t.shape[1] == 4
        cnt = np.zeros((len(t), B ** 3, n_classes), dtype=np.int64)
        have = t[:, 0] >= 0
        cnt[have] = v[t[have, 0]][:, :, :n_classes]
        return t, cnt.argmax(-1), cnt.sum(-1)

    def brick_labels(self, votes, table, n_classes, table_host=None):
        _, lab, n = self._decide(votes, table, n_classes)
        return torch.from_numpy(np.where(n > 0, lab, 255).astype(np.uint8).reshape(-1, B, B, B))

    def extract(self, votes, table, n_classes, min_obs=1, include_empty=False, table_host=None):
        t, lab, n = self._decide(votes, table, n_classes)
        keep = (n >= max(min_obs, 1)) & ((lab != 0) | bool(include_empty))
        b, vox = np.nonzero(keep)
        coords = (B * t[b, 1:4] + LOCAL[vox]).astype(np.int32)
        return (torch.from_numpy(coords), torch.from_numpy(lab[b, vox].astype(np.uint8)),
                torch.from_numpy(np.minimum(n[b, vox], 65535).astype(np.uint16).view(np.int16)))


def assert_map_equals_ref(m, ref):
    """Every brick of the map holds the restatement's votes; a brick the restatement never touched is all zero."""
    want = ref.bricks()
    keys = [tuple(k) for k in m.brick_keys().tolist()]
    assert set(want) <= set(keys) and len(set(keys)) == len(keys) == m.n_bricks
    votes = m.votes.cpu().numpy().view(np.uint16)
    slots = m.slots(np.array(keys))
    assert sorted(slots.tolist()) == list(range(len(keys)))
    for key, slot in zip(keys, slots):
        got = votes[slot].astype(np.int64)
        assert not got[..., m.n_classes:].any()
        expect = want.get(key)
        if expect is None:
            assert not got.any(), key
        else:
            assert np.array_equal(got[..., :m.n_classes], np.minimum(expect, 65535)), key
    if m.capacity > len(keys):
        assert not votes[len(keys):].any()


# ------------------------------------------------------------------------------------------------ coefficients
POSES = {"identity": pose(), "shift": pose(t=(0.4, -0.2, 0.2)), "yaw90": yaw90((0.2, 0.4, 0.0)),
         "generic": pose(17.3, 2.1, (1.13, -0.57, 0.21)), "generic2": pose(-31.7, -3.4, (-0.71, 0.93, -0.33))}


@pytest.mark.parametrize("name", sorted(POSES))
@pytest.mark.parametrize("dims", sorted(GRIDS))
def test_quantised_coefficients_stay_within_the_bound(name, dims):
    P, origin = POSES[name], GRIDS[dims]
    keys = sm.frame_bricks(P, origin, V, dims)
    Aq, cq = sm.brick_coefficients(P, keys, origin, V)
    assert Aq.dtype == cq.dtype == np.int32 and Aq.shape == (3, 3) and cq.shape == (len(keys), 3)
    rAq, rcq, c = ref_coefficients(P, keys, origin)
    assert np.array_equal(Aq, rAq) and np.array_equal(cq, rcq)          # the restatement's coefficients are the module's
    gq = LOCAL[None] @ rAq.T[None] + rcq[:, None, :]
    exact = LOCAL[None].astype(np.float64) @ P[:3, :3][None] + c[:, None, :]      # R^T (i, j, l) + c_k
    assert np.abs(gq / 65536.0 - exact).max() <= POS_TOL
    if name in ("identity", "shift", "yaw90"):
        assert np.array_equal(np.abs(Aq).sum(1), [65536] * 3)            # a signed permutation: exact


def test_far_bricks_are_refused():
    assert sm.brick_coefficients(pose(), [[1023, 0, 0]], (0.0, 0.0, 0.0), V)[1][0, 0] == (1023 * 16 << 16) + 32768
    with pytest.raises(ValueError, match="2\\^14"):
        sm.brick_coefficients(pose(), [[1024, 0, 0]], (0.0, 0.0, 0.0), V)      # c = 16384.5
    with pytest.raises(ValueError, match="2\\^14"):
        sm.brick_coefficients(pose(t=(0.0, 4000.0, 0.0)), [[0, 0, 0]], (0.0, 0.0, 0.0), V)


# ------------------------------------------------------------------------------------------------ brick selection
@pytest.mark.parametrize("dims", sorted(GRIDS))
def test_brick_selection_is_a_superset(dims):
    origin = GRIDS[dims]
    negative = False
    for P in sequence(dims):
        selected = {tuple(k) for k in sm.frame_bricks(P, origin, V, dims).tolist()}
        keys = generous_bricks(P, origin, dims, margin=2)
        Aq, cq, _ = ref_coefficients(P, keys, origin)
        idx = fixed_index(Aq, cq)
        inside = ((idx >= 0) & (idx < np.array(dims))).all(-1).any(1)
        assert inside.sum() * B ** 3 >= dims[0] * dims[1] * dims[2]
        needed = {tuple(k) for k in keys[inside].tolist()}
        assert needed <= selected
        assert len(selected) < len(keys)                                   # and it does select
        negative |= any(min(k) < 0 for k in needed)
    assert negative                                                        # floor, not truncation, is exercised


def test_keys_floor_and_pack_in_order():
    keys = np.array([[-2, 5, 0], [-1, -1, -1], [-1, 0, 3], [0, 0, 0], [0, 0, 1], [3, -7, 2]])
    p = sm.pack_keys(keys)
    assert list(p) == sorted(p) and np.array_equal(sm.unpack_keys(p), keys)
    # world voxel -1 lies in brick -1: an identity frame whose grid starts at -0.2 m
    k = sm.frame_bricks(pose(), (-0.2, 0.0, 0.0), V, (2, 1, 1))
    assert [-1, 0, 0] in k.tolist() and [0, 0, 0] in k.tolist()
    # a grid that lies on brick boundaries selects its own bricks and none that merely touch it
    assert sm.frame_bricks(pose(), (0.0, -1.6, 0.0), V, (32, 16, 16)).tolist() == [[0, -1, 0], [0, 0, 0], [1, -1, 0], [1, 0, 0]]
    with pytest.raises(ValueError):
        sm.pack_keys([[1 << 20, 0, 0]])


# ------------------------------------------------------------------------------------------------ directory and pool
def test_directory_pool_growth_limit_and_reset(monkeypatch):
    k = KernelStandIn().install(monkeypatch)
    dims, C = (16, 12, 8), 5
    origin = GRIDS[dims]
    m = sm.SemanticMap(C, V, origin, dims, chunk_bricks=4)
    assert (m.n_bricks, m.capacity, m.nbytes, m.pitch, m.brick_bytes) == (0, 0, 0, 8, 4096 * 8 * 2)
    assert m.brick_keys().shape == (0, 3) and m.extract()[0].shape == (0, 3)
    assert torch.equal(m.brick_labels([[0, 0, 0]]), torch.full((1, B, B, B), 255, dtype=torch.uint8))
    ref = MapRef(C, origin, dims)
    caps = []
    for (lab, mask), P in zip(frames_for(dims, C, 3, 6, masked=True), sequence(dims)):
        m.integrate(torch.from_numpy(lab), P, mask=torch.from_numpy(mask))
        ref.integrate(lab, P, mask)
        caps.append(m.capacity)
        assert m.capacity % 4 == 0 and m.capacity >= m.n_bricks and m.nbytes == m.capacity * m.brick_bytes
    assert caps == sorted(caps) and len(set(caps)) >= 3 and m.grown == len(set(caps))       # regrown between launches
    assert_map_equals_ref(m, ref)                                          # and the earlier votes came along
    assert len(k.calls) == 6 and all(c["mask"] for c in k.calls)
    # the same frame again: known bricks, no growth
    before = (m.n_bricks, m.grown)
    m.integrate(torch.from_numpy(frames_for(dims, C, 3, 1)[0][0]), pose())
    assert (m.n_bricks, m.grown) == before
    # max_bricks
    small = sm.SemanticMap(C, V, origin, dims, max_bricks=3, chunk_bricks=2)
    with pytest.raises(RuntimeError, match=r"max_bricks = 3 allows 0\.2 MB"):
        small.integrate(torch.zeros(dims, dtype=torch.uint8), pose())
    assert small.n_bricks == 0
    n_first = len(sm.frame_bricks(pose(), origin, V, dims))
    exact = sm.SemanticMap(C, V, origin, dims, max_bricks=n_first, chunk_bricks=1000)
    exact.integrate(torch.zeros(dims, dtype=torch.uint8), pose())
    assert exact.capacity == exact.n_bricks == n_first                    # the limit caps the chunk
    with pytest.raises(RuntimeError, match="max_bricks"):
        exact.integrate(torch.zeros(dims, dtype=torch.uint8), sequence(dims)[5])
    # reset
    cap = m.capacity
    m.reset()
    assert m.n_bricks == 0 and m.capacity == cap and not m.votes.any() and m.extract()[0].shape == (0, 3)
    m.integrate(torch.from_numpy(frames_for(dims, C, 3, 1)[0][0]), pose())
    assert_map_equals_ref(m, MapRef(C, origin, dims).integrate(frames_for(dims, C, 3, 1)[0][0], pose()))
    with pytest.raises(ValueError):
        m.integrate(torch.zeros((3, 3, 3), dtype=torch.uint8), pose())
    with pytest.raises(ValueError):
        sm.SemanticMap(33, V, origin, dims)


def test_extraction_on_the_stand_in_equals_the_restatement(monkeypatch):
    KernelStandIn().install(monkeypatch)
    dims, C = (16, 12, 8), 5
    origin = GRIDS[dims]
    m, ref = sm.SemanticMap(C, V, origin, dims, chunk_bricks=8), MapRef(C, origin, dims)
    for (lab, mask), P in zip(frames_for(dims, C, 4, 4), sequence(dims)):
        m.integrate(torch.from_numpy(lab), P)
        ref.integrate(lab, P)
    for min_obs, empty in ((1, False), (2, False), (1, True), (2, True), (50, True)):
        got, want = m.extract(min_obs, empty), ref.extract(min_obs, empty)
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
        assert np.array_equal(got[2].numpy().view(np.uint16), want[2])
        assert (len(want[1]) == 0) == (min_obs == 50)
    keys = m.brick_keys()
    lab = m.brick_labels(np.concatenate([keys, [[99, 99, 99]]])).numpy()
    assert all(np.array_equal(lab[i], ref.labels(k)) for i, k in enumerate(keys)) and (lab[-1] == 255).all()


# ------------------------------------------------------------------------------------------------ map_confusion
def _confusion_stand_in(hist, target, logits=None, labels=None):
    pred = labels if labels is not None else logits.argmax(1)
    t, p = target.reshape(-1).long(), pred.reshape(-1).long()
    keep = t != 255
    C = hist.shape[0]
    hist += torch.bincount(t[keep] * C + p[keep], minlength=C * C).reshape(C, C)
    return hist


def test_map_confusion_against_brute_force(monkeypatch):
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    KernelStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    dims, C = (16, 12, 8), 5
    origin = GRIDS[dims]
    maps = [sm.SemanticMap(C, V, origin, dims, chunk_bricks=8) for _ in range(2)]
    refs = [MapRef(C, origin, dims) for _ in range(2)]
    poses = sequence(dims)
    # the prediction sees frames 0..3 inside a mask, the ground truth frames 1..5 whole: neither covers the other
    for (lab, mask), P in zip(frames_for(dims, C, 5, 4, masked=True), poses[:4]):
        maps[0].integrate(torch.from_numpy(lab), P, mask=torch.from_numpy(mask))
        refs[0].integrate(lab, P, mask)
    for (lab, _), P in zip(frames_for(dims, C, 6, 5), poses[1:]):
        maps[1].integrate(torch.from_numpy(lab), P)
        refs[1].integrate(lab, P)
    want = confusion_ref(refs[0], refs[1], C)
    assert 0 < want.sum() < sum(1 for v in refs[1].votes.values() if v.sum() > 0) and (want - np.diag(np.diag(want))).any()
    for chunk in (512, 3):
        metric = sm.map_confusion(maps[0], maps[1], SSCMetrics(C, device="cpu"), chunk_bricks=chunk)
        assert np.array_equal(metric.hist.numpy(), want)
    with pytest.raises(ValueError, match="voxel sizes"):
        sm.map_confusion(maps[0], sm.SemanticMap(C, 0.4, origin, dims), SSCMetrics(C, device="cpu"))


# ------------------------------------------------------------------------------------------------ PLY
def test_ply_round_trip(tmp_path):
    from occdepth_amd import render
    coords = np.array([[-17, 3, 0], [0, 0, 0], [40, -2, 5]], dtype=np.int32)
    labels = np.array([1, 19, 7], dtype=np.uint8)
    n_obs = np.array([1, 65535, 300], dtype=np.uint16)
    pal = render.palette("kitti")
    path = sm.write_ply(str(tmp_path / "m.ply"), torch.from_numpy(coords), torch.from_numpy(labels),
                        torch.from_numpy(n_obs.view(np.int16)), V, pal)
    header = ("ply\nformat binary_little_endian 1.0\ncomment occdepth_amd semantic map voxel_size 0.2\nelement vertex 3\n"
              "property float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
              "property uchar blue\nproperty uchar label\nproperty ushort n_obs\nend_header\n").encode("ascii")
    data = open(path, "rb").read()
    assert data[:len(header)] == header and len(data) == len(header) + 3 * 18
    # the first vertex, byte by byte: three little-endian floats, rgb, label, n_obs
    first = np.array([(-17 + 0.5) * V, 3.5 * V, 0.5 * V], dtype="<f4").tobytes() + bytes(pal[1].tolist()) + bytes([1]) + b"\x01\x00"
    assert data[len(header):len(header) + 18] == first
    verts, v = sm.read_ply(path)
    assert v == V and len(verts) == 3
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], -1), ((coords + 0.5) * V).astype(np.float32))
    assert np.array_equal(verts["label"], labels) and np.array_equal(verts["n_obs"], n_obs)
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], -1), pal.numpy()[labels])
    empty = sm.write_ply(str(tmp_path / "e.ply"), coords[:0], labels[:0], n_obs[:0], V, pal)
    assert len(sm.read_ply(empty)[0]) == 0
    with pytest.raises(ValueError, match="colour"):
        sm.write_ply(str(tmp_path / "x.ply"), coords, np.array([1, 200, 7], dtype=np.uint8), n_obs, V, pal)
    with open(path, "ab") as f:
        f.write(b"\0")
    with pytest.raises(ValueError, match="announces"):
        sm.read_ply(path)


# ------------------------------------------------------------------------------------------------ the model hook
TR = "Tr: 0 -1 0 0.5 0 0 -1 0.25 1 0 0 -0.125"          # velodyne (x fwd, y left, z up) -> camera (x right, y down, z fwd)
HOOK_DIMS, HOOK_C = (8, 6, 4), 4
HOOK_ORIGIN = (0.0, -0.6, -0.4)


def _write_sequence(d, poses):
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "poses.txt"), "w") as f:
        f.write(poses)
    with open(os.path.join(d, "calib.txt"), "w") as f:
        f.write(TR + "\n")
    return str(d)


def _hook_stub(dataset="kitti", **extra):
    """The attribute set of the existing hook tests (tests/test_fuse.py): no `semantic_map` unless it is switched on."""
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    from occdepth_amd.models.OccDepth import OccDepth
    C = HOOK_C
    stub = SimpleNamespace(dataset=dataset, n_classes=C, full_scene_size=HOOK_DIMS, project_scale=1,
                           class_names=[str(i) for i in range(C)], metrics_allreduce=False, render=None,
                           report_metrics={}, temporal_fusion=None, fused_metrics={}, logged_keys={}, hists=[],
                           train_metrics=SSCMetrics(C, device="cpu"), val_metrics=SSCMetrics(C, device="cpu"),
                           test_metrics=SSCMetrics(C, device="cpu"), _kitti_origin=lambda batch=None: HOOK_ORIGIN, **extra)
    stub._report_fov = lambda batch, target: OccDepth._report_fov(stub, batch, target)
    stub._map_epoch_end = lambda step_type: OccDepth._map_epoch_end(stub, step_type)

    def epoch_stats(metric):
        stub.hists.append(None if metric.hist is None else metric.hist.clone())
        return metric.get_stats()
    stub._epoch_stats = epoch_stats
    stub._print_region_report = lambda prefix: print("region report")
    stub.log = lambda key, value, **kw: stub.logged_keys.__setitem__(key, value)
    return stub


def _hook_steps(seed=7):
    g = torch.Generator().manual_seed(seed)
    S = HOOK_DIMS[0] * HOOK_DIMS[1] * HOOK_DIMS[2]
    steps = []
    for seq, frames in (("08", (0, 1)), ("08", (2,)), ("03", (1,))):
        n = len(frames)
        batch = {"sequence": [seq] * n, "frame_id": ["%06d" % f for f in frames],
                 "fov_mask_1": [torch.rand(S, generator=g) < 0.7 for _ in frames]}
        target = torch.randint(0, HOOK_C, (n,) + HOOK_DIMS, generator=g).to(torch.uint8)
        target[:, 0, 0, 0] = 255
        steps.append((batch, torch.randn((n, HOOK_C) + HOOK_DIMS, generator=g) * 3, target))
    return steps


def _epoch(stub, step_type, steps):
    from occdepth_amd.models.OccDepth import OccDepth
    metric = getattr(stub, step_type + "_metrics")
    for batch, logits, target in steps:
        metric.add_batch_logits(logits, target)                            # what step() does with the ordinary metric
        if getattr(stub, "semantic_map", None) is not None:
            OccDepth._map_step(stub, step_type, batch, logits, target)
    (OccDepth.validation_epoch_end if step_type == "val" else OccDepth.test_epoch_end)(stub, [])


def test_model_hook_maps_scores_and_writes(monkeypatch, tmp_path, capsys):
    from occdepth_amd import fuse
    from occdepth_amd.models.OccDepth import OccDepth
    k = KernelStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    steps = _hook_steps()
    out_dir = tmp_path / "maps"

    # off: a stub WITHOUT the attribute, as the existing tests build it -- no key, no line, no file, no launch
    plain = _hook_stub()
    assert not hasattr(plain, "semantic_map")
    _epoch(plain, "val", steps)
    capsys.readouterr()
    _epoch(plain, "test", steps)
    lines_off = capsys.readouterr().out.splitlines()
    assert lines_off[0] == "test======" and lines_off[5:] == ["region report"] and len(lines_off) == 6
    assert not any("map" in key for key in plain.logged_keys) and not k.calls and not out_dir.exists()

    # on
    stub = _hook_stub(semantic_map=None)
    assert OccDepth.enable_semantic_map(stub, str(out_dir), str(root), min_obs=1) is stub
    _epoch(stub, "val", steps)
    assert set(stub.logged_keys) - set(plain.logged_keys) == {"val_map/mIoU", "val_map/IoU"}
    assert all(np.array_equal(stub.logged_keys[key], plain.logged_keys[key]) for key in plain.logged_keys)
    names = sorted(os.listdir(out_dir))
    assert names == ["val_03_gt.ply", "val_03_pred.ply", "val_08_gt.ply", "val_08_pred.ply"]
    assert stub.semantic_map["maps"] == {} and sorted(stub.semantic_map["poses"]) == ["03", "08"]    # released; poses read once
    assert len(k.calls) == 8 and all(c["mask"] for c in k.calls)           # 4 frames x (prediction, ground truth)
    assert [c["dtype"] for c in k.calls[:2]] == [torch.int16, torch.uint8]

    # the score is the brute-force confusion of the restatements, summed over the sequences; the files are their maps
    want = np.zeros((HOOK_C, HOOK_C), dtype=np.int64)
    vs = 0.2 * HOOK_DIMS[0] / HOOK_DIMS[0]
    for seq in ("03", "08"):
        poses = fuse.read_kitti_poses(str(root / seq))
        refs = [MapRef(HOOK_C, HOOK_ORIGIN, HOOK_DIMS, vs) for _ in range(2)]
        for batch, logits, target in steps:
            for i, s in enumerate(batch["sequence"]):
                if s == seq:
                    P, mask = poses[int(batch["frame_id"][i])], batch["fov_mask_1"][i].numpy()
                    refs[0].integrate(logits[i].argmax(0).numpy(), P, mask)
                    refs[1].integrate(target[i].numpy(), P, mask)
        want += confusion_ref(refs[0], refs[1], HOOK_C)
        for ref, name in zip(refs, ("pred", "gt")):
            verts, v = sm.read_ply(str(out_dir / ("val_%s_%s.ply" % (seq, name))))
            coords, labels, n_obs = ref.extract(1, False)
            assert v == vs and np.array_equal(verts["label"], labels) and np.array_equal(verts["n_obs"], n_obs)
            assert np.allclose(np.stack([verts["x"], verts["y"], verts["z"]], -1), (coords + 0.5) * vs, atol=1e-6)
    assert want.sum() > 0 and np.array_equal(stub.hists[-1].numpy(), want)

    # the test report: the block comes after the existing ones, in their five-line format
    capsys.readouterr()
    _epoch(stub, "test", steps[:2])
    out = capsys.readouterr().out.splitlines()
    assert out[:6] == lines_off[:1] + out[1:5] + ["region report"] and out[6] == "test_map======" and len(out) == 11
    assert [out[i].split("=")[0] for i in (1, 2, 4)] == [out[i].split("=")[0] for i in (7, 8, 10)]
    assert sorted(set(os.listdir(out_dir)) - set(names)) == ["test_08_gt.ply", "test_08_pred.ply"]
    # an epoch without frames prints and logs nothing more
    capsys.readouterr()
    OccDepth.test_epoch_end(stub, [])
    assert "map" not in capsys.readouterr().out
    with pytest.raises(KeyError, match="poses.txt"):
        OccDepth._map_step(stub, "val", {"sequence": ["08"], "frame_id": ["000009"]}, steps[1][1], steps[1][2])


def test_enable_semantic_map_refusals(tmp_path):
    from occdepth_amd.models.OccDepth import OccDepth
    with pytest.raises(NotImplementedError, match="SemanticKITTI"):
        OccDepth.enable_semantic_map(_hook_stub(dataset="NYU"), str(tmp_path), str(tmp_path))
    with pytest.raises(ValueError, match="OCCDEPTH_MAP_POSES"):
        OccDepth.enable_semantic_map(_hook_stub(), str(tmp_path), "")
    with pytest.raises(ValueError, match="OCCDEPTH_MAP_DIR"):
        OccDepth.enable_semantic_map(_hook_stub(), "", str(tmp_path))
    with pytest.raises(ValueError, match="min_obs"):
        OccDepth.enable_semantic_map(_hook_stub(), str(tmp_path), str(tmp_path), min_obs=0)
    stub = OccDepth.enable_semantic_map(_hook_stub(), str(tmp_path / "out"), str(tmp_path / "nowhere"))
    with pytest.raises(FileNotFoundError, match="calib.txt"):              # a poses root without the sequence
        OccDepth._map_step(stub, "val", {"sequence": ["08"], "frame_id": ["000000"]},
                           torch.zeros((1, HOOK_C) + HOOK_DIMS), torch.zeros((1,) + HOOK_DIMS, dtype=torch.uint8))


def test_model_map_is_off_by_default_and_switched_by_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def model(name):
        cfg, _ = gc.occdepth_config(name)
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg)

    for var in ("OCCDEPTH_MAP_DIR", "OCCDEPTH_MAP_POSES", "OCCDEPTH_MAP_MIN_OBS", "OCCDEPTH_FUSE", "OCCDEPTH_FUSE_POSES"):
        monkeypatch.delenv(var, raising=False)
    assert model("kitti_flosp_small").semantic_map is None
    monkeypatch.setenv("OCCDEPTH_MAP_DIR", str(tmp_path / "maps"))
    with pytest.raises(ValueError, match="OCCDEPTH_MAP_POSES"):
        model("kitti_flosp_small")
    monkeypatch.setenv("OCCDEPTH_FUSE_POSES", str(tmp_path / "fuse"))      # the fall-back
    assert model("kitti_flosp_small").semantic_map["poses_root"] == str(tmp_path / "fuse")
    monkeypatch.setenv("OCCDEPTH_MAP_POSES", str(tmp_path / "seq"))
    monkeypatch.setenv("OCCDEPTH_MAP_MIN_OBS", "2")
    st = model("kitti_flosp_small").semantic_map
    assert (st["out_dir"], st["poses_root"], st["min_obs"], st["maps"]) == (str(tmp_path / "maps"), str(tmp_path / "seq"), 2, {})
    assert not (tmp_path / "maps").exists()                                # nothing is written before an epoch ends
    with pytest.raises(NotImplementedError):
        model("nyu_small")


# ------------------------------------------------------------------------------------------------ argument checks
def test_map_entry_points_validate_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected
    host16 = np.zeros((2, 16), dtype=np.int32)
    host4 = np.zeros((2, 4), dtype=np.int32)

    def frame():
        a = hip.MapFrameArgs()
        a.votes = a.table = a.labels = ptr
        a.n_bricks, a.capacity, a.X, a.Y, a.Z, a.C, a.pitch, a.label_bytes = 2, 4, 40, 24, 20, 20, 20, 1
        return a

    integrate = hip_lib.occd_map_integrate
    assert integrate(None, None) == -1
    for field, value in (("votes", None), ("table", None), ("labels", None), ("C", 0), ("C", 33), ("X", 0), ("Y", -1),
                         ("Z", 0), ("n_bricks", 0), ("n_bricks", -3), ("capacity", 0), ("label_bytes", 0),
                         ("label_bytes", 3), ("label_bytes", 4), ("pitch", 19), ("pitch", 16), ("pitch", 22), ("pitch", 0),
                         ("votes", ptr + 2)):
        a = frame()
        setattr(a, field, value)
        assert integrate(ctypes.byref(a), None) == -1, (field, value)
    a = frame()
    a.X = a.Y = a.Z = 1 << 10                                              # 2^30 voxels
    assert integrate(ctypes.byref(a), None) == -1
    for slot in (4, 1 << 20, -1):                                          # a slot at or past the capacity, or none
        a = frame()
        host16[1, 0] = slot
        a.table_host = host16.ctypes.data
        assert integrate(ctypes.byref(a), None) == -1, slot

    def extract():
        a = hip.MapExtractArgs()
        a.votes = a.table = a.dense = a.counts = a.offsets = a.coords = a.labels = a.n_obs = ptr
        a.n_out, a.n_bricks, a.capacity, a.C, a.pitch, a.min_obs, a.include_empty = 5, 2, 4, 20, 20, 1, 0
        return a

    common = (("votes", None), ("table", None), ("C", 0), ("C", 33), ("n_bricks", 0), ("n_bricks", -1), ("capacity", 0),
              ("capacity", -2), ("pitch", 19), ("pitch", 16), ("pitch", 22), ("min_obs", -1), ("votes", ptr + 4))
    own = {"occd_map_brick_labels": (("dense", None),), "occd_map_count": (("counts", None),),
           "occd_map_extract": (("offsets", None), ("coords", None), ("labels", None), ("n_obs", None), ("n_out", 0),
                                ("n_out", -1))}
    for name, cases in own.items():
        fn = getattr(hip_lib, name)
        assert fn(None, None) == -1
        for field, value in common + cases:
            a = extract()
            setattr(a, field, value)
            assert fn(ctypes.byref(a), None) == -1, (name, field, value)
        a = extract()
        host4[0, 0] = 4                                                    # a negative slot is a brick that is not there: allowed
        a.table_host = host4.ctypes.data
        assert fn(ctypes.byref(a), None) == -1, name
    assert hip.ABI_VERSION == 22 and hip.MAP_BRICK == 16
    assert ctypes.sizeof(hip.MapFrameArgs) == 5 * 8 + 8 * 4 and ctypes.sizeof(hip.MapExtractArgs) == 9 * 8 + 8 + 6 * 4
    for name in ("occd_map_integrate", "occd_map_brick_labels", "occd_map_count", "occd_map_extract"):
        assert name in hip.EXPORTS


# ------------------------------------------------------------------------------------------------ the offline tool
def _tool():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "map_sequence.py")
    spec = importlib.util.spec_from_file_location("map_sequence_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_map_sequence_tool_reads_pickles_and_submission_labels(monkeypatch, tmp_path, capsys):
    import pickle
    from occdepth_amd import output
    tool = _tool()
    KernelStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    lut = tool.submission_inverse_lut()
    assert [int(lut[v]) for v in output.KITTI_LEARNING_MAP_INV] == list(range(20)) and lut[1] == 255 and lut[252] == 255
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    seq = _write_sequence(tmp_path / "08", "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 0.4\n1 0 0 0.2 0 1 0 0 0 0 1 1.0\n")
    frames = frames_for(dims, C, 21, 3, masked=True)
    pkl, sub = tmp_path / "pkl", tmp_path / "sub"
    os.makedirs(pkl)
    os.makedirs(sub)
    for n, (lab, mask) in enumerate(frames):
        target = np.roll(lab, 1, axis=0)
        with open(pkl / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": lab.astype(np.uint16), "target": target.astype(np.uint16), "fov_mask_1": mask.reshape(-1)}, f)
        ids = np.array(output.KITTI_LEARNING_MAP_INV + (999,) * 236, dtype=np.uint16)[lab]      # 255 / C -> an unknown id
        ids.reshape(-1).tofile(str(sub / ("%06d.label" % n)))
    assert tool.list_frames(str(pkl))[0] == "pkl" and tool.list_frames(str(sub))[0] == "label"
    with pytest.raises(FileNotFoundError):
        tool.list_frames(str(tmp_path))
    args = tool.parser().parse_args(["--poses", seq, "--pred", str(sub), "--gt", str(pkl), "--out", str(tmp_path / "m" / "08"),
                                     "--dims", "16", "12", "8", "--origin"] + [str(o) for o in origin] + ["--fov"])
    maps, stats = tool.run(args, device=torch.device("cpu"))
    from occdepth_amd import fuse
    poses = fuse.read_kitti_poses(seq)
    refs = [MapRef(C, origin, dims), MapRef(C, origin, dims)]
    for n, (lab, mask) in enumerate(frames):
        refs[0].integrate(lab, poses[n])                                   # submission files carry no mask
        refs[1].integrate(np.roll(lab, 1, axis=0), poses[n], mask)
    assert_map_equals_ref(maps["pred"], refs[0])
    assert_map_equals_ref(maps["gt"], refs[1])
    verts, v = sm.read_ply(str(tmp_path / "m" / "08_pred.ply"))
    assert v == V and np.array_equal(verts["label"], refs[0].extract(1, False)[1])
    assert len(sm.read_ply(str(tmp_path / "m" / "08_gt.ply"))[0]) == len(refs[1].extract(1, False)[1])
    out = capsys.readouterr().out
    assert "map======" in out and "mIoU=" in out and stats["iou_ssc_mean"] >= 0
