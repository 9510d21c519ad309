"""CPU: the map read back into a frame (K32, occd_map_sample) -- `sample_ref`, the numpy int64 restatement of the kernel
on top of `MapRef` (tests/test_map.py): it knows the fixed-point arithmetic of the header and nothing of bricks, tables
or windows (tests/test_map_sample_gpu.py holds the kernel to it with exact equality); the quantised coefficients against
float64, the window, the refusals, exact self-exclusion, SemanticMap.sample with the kernel replaced by a stand-in that
works from the tables the host side builds, the model hook, the offline tool, and the argument checks of the entry point
before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd import semantic_map as sm
from test_map import (B, GRIDS, HOOK_C, HOOK_DIMS, HOOK_ORIGIN, V, KernelStandIn, MapRef, _confusion_stand_in, _epoch,
                      _hook_steps, _hook_stub, _tool, _write_sequence, frames_for, pose, ref_coefficients, sequence,
                      voting_labels, yaw90)


# ------------------------------------------------------------------------------------------------ the restatement
def lattice(dims):
    """(X Y Z, 3) int64: the frame voxels in flat order, z fastest."""
    return np.stack(np.meshgrid(*(np.arange(d) for d in dims), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def ref_window(P, origin, dims, v=V):
    """key_min, key_max (3,) int64: the brick range of the grid's corners in world voxels, a voxel wider on every side."""
    corners = np.array([[x, y, z] for x in (0.0, dims[0]) for y in (0.0, dims[1]) for z in (0.0, dims[2])])
    world = ((corners * v + np.asarray(origin, dtype=np.float64)) @ P[:3, :3].T + P[:3, 3]) / v
    return ((np.floor(world.min(0)) - 1.0) // B).astype(np.int64), ((np.floor(world.max(0)) + 1.0) // B).astype(np.int64)


def ref_sample_coefficients(P, origin, key_min, v=V):
    """Bq (3, 3), dq (3,) as int64 and d in float64: d = R (1/2 + o / v) + t / v - 16 key_min."""
    R, t = P[:3, :3], P[:3, 3]
    d = R @ (0.5 + np.asarray(origin, dtype=np.float64) / v) + t / v - float(B) * np.asarray(key_min, dtype=np.float64)
    return np.rint(R * 65536.0).astype(np.int64), np.rint(d * 65536.0).astype(np.int64), d


def world_voxels(P, origin, dims, v=V):
    """(X Y Z, 3) int64: the world voxel every frame voxel falls into, by the header's fixed point."""
    key_min, _ = ref_window(P, origin, dims, v)
    Bq, dq, _ = ref_sample_coefficients(P, origin, key_min, v)
    wq = lattice(dims) @ Bq.T + dq
    assert np.abs(wq).max() < 2 ** 31
    return (wq >> 16) + B * key_min


def own_votes(P, origin, dims, C, world, own, own_mask, v=V):
    """(n,) int64: the class this frame's integrate left a vote for in each world voxel (by integrate's own arithmetic:
    the brick's c_k, the local voxel, gq >> 16), -1 where it left none."""
    key, loc = world // B, world % B
    Aq, cq, _ = ref_coefficients(P, key, origin, v)
    idx = (loc @ Aq.T + cq) >> 16
    return voting_labels(idx[None], own, own_mask, dims, C)[0]


def decide_ref(cnt, own, vote, dims, C, min_obs, exclude_self, keep_own):
    """cnt (S, C) int64 saturated counters, own (S,) int64 or None, vote (S,) int64 (own_votes) -> labels, n_obs."""
    cnt = cnt.copy()
    S = len(cnt)
    if exclude_self:
        s = np.nonzero(vote >= 0)[0]
        cur = cnt[s, vote[s]]
        cnt[s, vote[s]] = cur - ((cur != 0) & (cur != 65535))
    n, best, lab = cnt.sum(-1), cnt.max(-1), cnt.argmax(-1)               # np.argmax: the lowest class on a tie
    if keep_own:
        mine = cnt[np.arange(S), np.clip(own, 0, C - 1)]
        lab = np.where((own < C) & (mine == best) & (best > 0), own, lab)
    fallback = np.full(S, 255) if own is None else np.minimum(own, 255)
    labels = np.where(n >= max(min_obs, 1), lab, fallback).astype(np.uint8).reshape(dims)
    return labels, np.minimum(n, 65535).astype(np.uint16).reshape(dims)


def _flat(own):
    return None if own is None else np.asarray(own).reshape(-1).astype(np.int64)


def ref_counters(map_ref, P):
    """(world (S, 3), cnt (S, C)): the saturated counters under every frame voxel; kept per pose until the map changes."""
    bricks = map_ref.bricks()
    cache = getattr(map_ref, "_sample_cache", None)
    if cache is None or cache[0] is not bricks:
        cache = map_ref._sample_cache = (bricks, {})
    key = np.asarray(P, dtype=np.float64).tobytes()
    if key not in cache[1]:
        world = world_voxels(P, map_ref.origin, map_ref.dims, map_ref.v)
        bk, loc = world // B, world % B
        cnt = np.zeros((len(world), map_ref.C), dtype=np.int64)
        uniq, inv = np.unique(bk, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        for u, k in enumerate(uniq.tolist()):
            brick = bricks.get(tuple(k))
            if brick is not None:
                sel = inv == u
                cnt[sel] = brick[loc[sel, 0], loc[sel, 1], loc[sel, 2]]
        cache[1][key] = (world, np.minimum(cnt, 65535))
    return cache[1][key]


def sample_ref(map_ref, pose, own=None, own_mask=None, min_obs=1, exclude_self=False, keep_own=False):
    """occd_map_sample restated -> labels (X, Y, Z) uint8, n_obs (X, Y, Z) uint16.  own: uint8 / uint16 VALUES."""
    world, cnt = ref_counters(map_ref, pose)
    vote = None
    if exclude_self:
        vote = own_votes(pose, map_ref.origin, map_ref.dims, map_ref.C, world, own, own_mask, map_ref.v)
    return decide_ref(cnt, _flat(own), vote, map_ref.dims, map_ref.C, min_obs, exclude_self, keep_own)


# ------------------------------------------------------------------------------------------------ the kernel stand-in
class SampleStandIn:
    """hip.map_sample on CPU tensors, from the directory, the table and the coefficients the host side hands over."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "map_sample", self.sample)
        return self

    def sample(self, votes, table, cells, own, dims, n_classes, Bq, dq, grid, own_mask=None, min_obs=1, exclude_self=False,
               keep_own=False, table_host=None):
        v, t, cl = KernelStandIn._u16(votes), table.numpy().astype(np.int64), cells.numpy().astype(np.int64)
        assert t.shape[1] == 16 and len(t) and t[:, 0].min() >= 0 and t[:, 0].max() < len(v)      # only bricks of the map
        assert table_host is not None and torch.equal(table_host, table) and cl.shape == tuple(grid)
        assert sorted(cl[cl >= 0].tolist()) == list(range(len(t)))         # every row sits in exactly one cell
        assert own is not None or not (exclude_self or keep_own)
        self.calls.append({"n": len(t), "mask": own_mask is not None, "exclude_self": exclude_self, "keep_own": keep_own,
                           "min_obs": min_obs})
        C, S = n_classes, dims[0] * dims[1] * dims[2]
        wq = lattice(dims) @ np.asarray(Bq, dtype=np.int64).T + np.asarray(dq, dtype=np.int64)
        assert np.abs(wq).max() < 2 ** 31
        idx = wq >> 16
        cell, loc = idx >> 4, idx & 15
        inside = ((cell >= 0) & (cell < np.array(grid))).all(-1)
        cell = np.clip(cell, 0, np.array(grid) - 1)
        row = np.where(inside, cl[cell[:, 0], cell[:, 1], cell[:, 2]], -1)
        have = row >= 0
        cnt = np.zeros((S, C), dtype=np.int64)
        cnt[have] = v[t[row[have], 0], (loc[have, 0] * B + loc[have, 1]) * B + loc[have, 2], :C]
        flat = None
        if own is not None:
            flat = own.numpy().reshape(-1)
            flat = (flat.view(np.uint16) if flat.dtype == np.int16 else flat).astype(np.int64)
        vote = np.full(S, -1, dtype=np.int64)
        if exclude_self:
            m = None if own_mask is None else own_mask.numpy().reshape(-1)
            r = t[row[have]]
            gq = (r[:, 4:13].reshape(-1, 3, 3) * loc[have][:, None, :]).sum(-1) + r[:, 13:16]
            vote[have] = voting_labels((gq >> 16)[None], flat, m, dims, C)[0]
        labels, n_obs = decide_ref(cnt, flat, vote, tuple(dims), C, min_obs, exclude_self, keep_own)
        return torch.from_numpy(labels), torch.from_numpy(n_obs.view(np.int16))


# ------------------------------------------------------------------------------------------------ coefficients
SHIFT = np.array([0.03, 0.05, 0.07])            # metres: takes the lattices of the axis-aligned poses off the voxel boundaries


@pytest.mark.parametrize("dims", sorted(GRIDS))
def test_fixed_point_world_voxel_equals_float64_floor(dims):
    origin = tuple(np.asarray(GRIDS[dims]) + SHIFT)
    G = lattice(dims).astype(np.float64)
    tol = (sum(dims) + 1) * 2.0 ** -17          # rounding Bq (X + Y + Z half-ulps at most) and dq (one)
    for P in sequence(dims):
        key_min, key_max = sm.frame_brick_box(P, origin, V, dims)
        assert np.array_equal(key_min, ref_window(P, origin, dims)[0]) and np.array_equal(key_max, ref_window(P, origin, dims)[1])
        Bq, dq = sm.sample_coefficients(P, origin, V, key_min, dims)
        rBq, rdq, d = ref_sample_coefficients(P, origin, key_min)
        assert Bq.dtype == dq.dtype == np.int32 and Bq.shape == (3, 3) and dq.shape == (3,)
        assert np.array_equal(Bq, rBq) and np.array_equal(dq, rdq)        # the restatement's coefficients are the module's
        exact = G @ P[:3, :3].T + d                                        # world position relative to 16 key_min, float64
        fixed = (lattice(dims) @ rBq.T + rdq)
        assert np.abs(fixed / 65536.0 - exact).max() <= tol
        near = (np.abs(exact - np.rint(exact)) < tol).any(1)
        assert near.mean() <= 0.02, near.mean()                            # the float64 reference alone stays under the cap
        assert np.array_equal((fixed >> 16)[~near], np.floor(exact).astype(np.int64)[~near])
        if np.array_equal(np.abs(rBq).sum(1), [65536] * 3):                # a signed permutation: no voxel is near a boundary
            assert not near.any()


@pytest.mark.parametrize("dims", sorted(GRIDS))
def test_every_frame_voxel_falls_inside_the_window(dims):
    origin = GRIDS[dims]
    extra = [pose(45.0, 0.0, (3.3, -7.1, 0.4)), pose(-120.0, 4.0, (-9.7, 2.2, -0.6)), yaw90((-0.2, 0.6, 0.2))]
    for P in sequence(dims) + extra:
        key_min, key_max = sm.frame_brick_box(P, origin, V, dims)
        cell = (world_voxels(P, origin, dims) - B * key_min) >> 4
        assert cell.min() >= 0 and (cell <= key_max - key_min).all()
        culled = sm.frame_bricks(P, origin, V, dims)                       # and the culled list lies inside the box
        assert (culled >= key_min).all() and (culled <= key_max).all()


def test_refusals():
    with pytest.raises(ValueError, match="2\\^14"):
        sm.sample_coefficients(pose(), (0.0, 0.0, 0.0), V, (0, 0, 0), dims=(1 << 13, 1 << 13, 1))
    assert sm.sample_coefficients(pose(), (0.0, 0.0, 0.0), V, (0, 0, 0), dims=(1 << 13, (1 << 13) - 2, 1))[1].tolist() == [32768] * 3
    with pytest.raises(ValueError, match="2\\^14"):
        sm.sample_coefficients(pose(), (0.0, 0.0, 0.0), V, (-1024, 0, 0))  # d = 16384.5
    assert sm.sample_coefficients(pose(), (0.0, 0.0, 0.0), V, (-1023, 0, 0))[1][0] == (1023 * 16 << 16) + 32768
    with pytest.raises(ValueError, match="2\\^14"):
        sm.sample_coefficients(pose(t=(0.0, 4000.0, 0.0)), (0.0, 0.0, 0.0), V, (0, 0, 0))
    m = sm.SemanticMap(5, V, GRIDS[(16, 12, 8)], (16, 12, 8))
    for flags in ({"exclude_self": True}, {"keep_own": True}):
        with pytest.raises(ValueError, match="own"):
            m.sample(pose(), **flags)
        with pytest.raises(RuntimeError, match="own"):
            hip.map_sample(torch.zeros((1, B ** 3, 8), dtype=torch.int16), torch.zeros((1, 16), dtype=torch.int32),
                           torch.zeros((1, 1, 1), dtype=torch.int32), None, (16, 12, 8), 5, np.eye(3, dtype=np.int32),
                           np.zeros(3, dtype=np.int32), (1, 1, 1), **flags)
    with pytest.raises(ValueError, match="min_obs"):
        m.sample(pose(), min_obs=-1)
    with pytest.raises(ValueError, match="2\\^14"):
        sm.SemanticMap(5, V, (0.0, 0.0, 0.0), (1 << 13, 1 << 13, 1)).sample(pose())


# ------------------------------------------------------------------------------------------------ self-exclusion
@pytest.mark.parametrize("masked", [False, True])
def test_exclude_self_equals_the_map_of_the_other_frames(masked):
    dims, C = (16, 12, 8), 5
    origin = GRIDS[dims]
    frames, poses = frames_for(dims, C, 31, 6, masked=masked), sequence(dims)
    whole, others = MapRef(C, origin, dims), MapRef(C, origin, dims)
    for i, ((lab, mask), P) in enumerate(zip(frames, poses)):
        whole.integrate(lab, P, mask)
        if i != 3:
            others.integrate(lab, P, mask)
    assert max(int(v.max()) for v in whole.votes.values()) < 65535         # no counter saturates at these sizes
    own, mask = frames[3]
    for keep_own in (False, True):
        for min_obs in (1, 2):
            got = sample_ref(whole, poses[3], own, mask, min_obs, exclude_self=True, keep_own=keep_own)
            want = sample_ref(others, poses[3], own, mask, min_obs, exclude_self=False, keep_own=keep_own)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    kept = sample_ref(whole, poses[3], own, mask)
    assert (kept[1] > want[1]).any() and (kept[1] >= want[1]).all()        # and without the flag the vote is there


# ------------------------------------------------------------------------------------------------ SemanticMap.sample
@pytest.mark.parametrize("dims,C,label_bytes,masked", [((16, 12, 8), 5, 1, True), ((40, 24, 20), 7, 2, False)])
def test_sample_on_the_stand_in_equals_the_restatement(monkeypatch, dims, C, label_bytes, masked):
    KernelStandIn().install(monkeypatch)
    k = SampleStandIn().install(monkeypatch)
    origin = GRIDS[dims]
    m, ref = sm.SemanticMap(C, V, origin, dims, chunk_bricks=8), MapRef(C, origin, dims)
    frames, poses = frames_for(dims, C, 41, 6, label_bytes, masked), sequence(dims)

    def tensor(lab):
        return torch.from_numpy(lab if lab.dtype == np.uint8 else lab.view(np.int16))

    # an empty map: the fallback volume and zeros, no launch
    lab, n = m.sample(poses[0], own=tensor(frames[0][0]))
    assert np.array_equal(lab.numpy(), np.minimum(frames[0][0], 255).astype(np.uint8)) and not n.any() and n.dtype == torch.int16
    lab, n = m.sample(poses[0])
    assert (lab == 255).all() and lab.dtype == torch.uint8 and tuple(lab.shape) == dims and not k.calls
    for (lab, mask), P in zip(frames[:5], poses):
        m.integrate(tensor(lab), P, mask=None if mask is None else torch.from_numpy(mask))
        ref.integrate(lab, P, mask)
    before = (m.votes.clone(), m.n_bricks, m.capacity)
    for i, P in enumerate(poses[:5]):
        own, mask = frames[i]
        for flags in ((False, False), (True, False), (False, True), (True, True)):
            got = m.sample(P, own=tensor(own), own_mask=None if mask is None else torch.from_numpy(mask), min_obs=1 + i % 2,
                           exclude_self=flags[0], keep_own=flags[1])
            want = sample_ref(ref, P, own, mask, 1 + i % 2, *flags)
            assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy().view(np.uint16), want[1]), (i, flags)
    # a frame that meets no brick of the map -- no launch, none admitted
    calls = len(k.calls)
    lab, n = m.sample(pose(5.2, 0.7, (60.0, 0.3, 0.1)), own=tensor(frames[5][0]))
    assert len(k.calls) == calls and not n.any() and np.array_equal(lab.numpy(), np.minimum(frames[5][0], 255).astype(np.uint8))
    assert torch.equal(m.votes, before[0]) and (m.n_bricks, m.capacity) == before[1:]
    # one that meets only some
    part = pose(9.0, 1.0, (dims[0] * V * 0.6, 0.2, 0.1))
    got, want = m.sample(part), sample_ref(ref, part)
    assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy().view(np.uint16), want[1])
    assert (want[1] == 0).any() and (want[1] > 0).any() and (want[0][want[1] == 0] == 255).all()
    cells, table, key_min = m.frame_cells(part, "cpu")
    assert cells.dtype == table.dtype == np.int32 and (cells < 0).any() and table.shape == ((cells >= 0).sum(), 16)
    with pytest.raises(ValueError):
        m.sample(poses[0], own=torch.zeros((3, 3, 3), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the model hook
def _hook_world(tmp_path):
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    return root


def _install_hook_stand_ins(monkeypatch):
    k = KernelStandIn().install(monkeypatch)
    s = SampleStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    return k, s


def test_model_hook_scores_and_writes_the_mapped_frames(monkeypatch, tmp_path, capsys):
    from occdepth_amd import fuse, output
    from occdepth_amd.models.OccDepth import OccDepth
    _, s = _install_hook_stand_ins(monkeypatch)
    root, steps = _hook_world(tmp_path), _hook_steps()
    returned = {}

    def recording(stub, name):
        def end(step_type):
            returned[name] = OccDepth._map_epoch_end(stub, step_type)
            return returned[name]
        stub._map_epoch_end = end

    # frames off: nothing is kept, sampled or logged, and the map's own statistics are the yardstick for below
    off = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps_off"), str(root), min_obs=1)
    recording(off, "off")
    _epoch(off, "val", steps)
    assert off.semantic_map["frames"] is False and off.semantic_map["kept"] == {} and not s.calls
    assert not any("mapped" in key for key in off.logged_keys) and "val_map/mIoU" in off.logged_keys
    capsys.readouterr()
    _epoch(off, "test", steps)
    out_off = capsys.readouterr().out.splitlines()
    assert "test_map======" in out_off and "test_mapped======" not in out_off and not s.calls

    # on
    sub = tmp_path / "submission"
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps"), str(root), min_obs=1, frames=True,
                                        submission_dir=str(sub))
    recording(stub, "on")
    for batch, logits, target in steps[:1]:                                # mid-epoch: the frames are kept, nothing sampled yet
        OccDepth._map_step(stub, "val", batch, logits, target)
    kept = stub.semantic_map["kept"][("val", "08")]
    assert len(kept) == 2 and kept[0][0].dtype == kept[0][1].dtype == torch.uint8 and tuple(kept[0][0].shape) == HOOK_DIMS
    assert kept[1][4] == "000001" and kept[0][2].dtype == torch.bool and not s.calls
    stub.semantic_map["maps"].clear()
    stub.semantic_map["kept"].clear()
    _epoch(stub, "val", steps)
    assert set(stub.logged_keys) - set(off.logged_keys) == {"val_mapped/mIoU", "val_mapped/IoU"}
    assert all(np.array_equal(stub.logged_keys[key], off.logged_keys[key]) for key in off.logged_keys)
    assert stub.semantic_map["kept"] == {} and stub.semantic_map["maps"] == {} and stub.semantic_map["mapped_stats"] == {}
    assert len(s.calls) == 4 and all(c["keep_own"] and not c["exclude_self"] and c["mask"] and c["min_obs"] == 1 for c in s.calls)

    # the score is the brute-force confusion of the restatement's mapped frames against their targets; the files hold them
    want = np.zeros((HOOK_C, HOOK_C), dtype=np.int64)
    ids = np.array(output.KITTI_LEARNING_MAP_INV, dtype=np.uint16)
    vs = 0.2
    n_files = 0
    for seq in ("03", "08"):
        poses = fuse.read_kitti_poses(str(root / seq))
        ref = MapRef(HOOK_C, HOOK_ORIGIN, HOOK_DIMS, vs)
        mine = [(logits[i].argmax(0).numpy().astype(np.uint8), target[i].numpy(), batch["fov_mask_1"][i].numpy(),
                 poses[int(batch["frame_id"][i])], batch["frame_id"][i])
                for batch, logits, target in steps for i, q in enumerate(batch["sequence"]) if q == seq]
        for pred, _, mask, P, _ in mine:
            ref.integrate(pred, P, mask)
        for pred, target, mask, P, frame_id in mine:
            mapped, _ = sample_ref(ref, P, pred, mask, 1, False, True)
            keep = target != 255
            np.add.at(want, (target[keep].astype(np.int64), mapped[keep].astype(np.int64)), 1)
            path = sub / "sequences" / seq / "predictions" / (frame_id + ".label")
            data = np.fromfile(str(path), dtype=np.uint16)
            assert data.shape == (mapped.size,) and np.array_equal(data, ids[mapped.reshape(-1)])      # dataset ids, (X, Y, Z) order
            n_files += 1
    assert n_files == 4 and want.sum() > 0 and np.array_equal(stub.hists[-2].numpy(), want)
    # _map_epoch_end returns what it returned before
    assert sorted(returned["on"]) == sorted(returned["off"])
    assert all(np.array_equal(returned["on"][key], returned["off"][key]) for key in returned["off"])

    # the test report: the mapped block follows the map block, in the same five-line format
    capsys.readouterr()
    _epoch(stub, "test", steps)
    out = capsys.readouterr().out.splitlines()
    assert out[:len(out_off)] == out_off and out[len(out_off)] == "test_mapped======" and len(out) == len(out_off) + 5
    at = out_off.index("test_map======")
    assert [out[at + i].split("=")[0] for i in (1, 2, 4)] == [out[len(out_off) + i].split("=")[0] for i in (1, 2, 4)]

    # exclude_self reaches the kernel; max_frames raises before anything is kept or launched
    s.calls.clear()
    excl = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps_x"), str(root), frames=True,
                                        exclude_self=True)
    _epoch(excl, "val", steps[:1])
    assert len(s.calls) == 2 and all(c["exclude_self"] and c["keep_own"] for c in s.calls)
    assert not (tmp_path / "maps_x" / "sequences").exists()
    small = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps_s"), str(root), frames=True, max_frames=2)
    OccDepth._map_step(small, "val", *steps[0])
    with pytest.raises(RuntimeError, match="max_frames = 2"):
        OccDepth._map_step(small, "val", *steps[1])
    assert sum(len(v) for v in small.semantic_map["kept"].values()) == 2
    with pytest.raises(ValueError, match="max_frames"):
        OccDepth.enable_semantic_map(_hook_stub(), str(tmp_path), str(root), frames=True, max_frames=0)


def test_map_frames_are_switched_by_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def state():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg).semantic_map

    for var in ("OCCDEPTH_MAP_FRAMES", "OCCDEPTH_MAP_FRAMES_SELF", "OCCDEPTH_MAP_SUBMISSION", "OCCDEPTH_MAP_MIN_OBS",
                "OCCDEPTH_MAP_VIEWS", "OCCDEPTH_FUSE", "OCCDEPTH_FUSE_POSES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OCCDEPTH_MAP_DIR", str(tmp_path / "maps"))
    monkeypatch.setenv("OCCDEPTH_MAP_POSES", str(tmp_path / "seq"))
    st = state()
    assert (st["frames"], st["exclude_self"], st["submission_dir"], st["kept"]) == (False, False, None, {})
    monkeypatch.setenv("OCCDEPTH_MAP_FRAMES", "1")
    st = state()
    assert (st["frames"], st["exclude_self"], st["submission_dir"]) == (True, False, None)
    monkeypatch.setenv("OCCDEPTH_MAP_FRAMES_SELF", "0")
    assert state()["exclude_self"] is True
    monkeypatch.setenv("OCCDEPTH_MAP_FRAMES_SELF", "1")
    monkeypatch.delenv("OCCDEPTH_MAP_FRAMES")
    monkeypatch.setenv("OCCDEPTH_MAP_SUBMISSION", str(tmp_path / "sub"))
    st = state()
    assert (st["frames"], st["exclude_self"], st["submission_dir"]) == (True, False, str(tmp_path / "sub"))
    assert not (tmp_path / "sub").exists()


def test_submission_labels_are_dataset_ids(tmp_path):
    from occdepth_amd import output
    lab = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    lab[1, 2, 3] = 255
    path = output.write_kitti_submission_labels(torch.from_numpy(lab), "08", "000123", str(tmp_path))
    assert path == str(tmp_path / "sequences" / "08" / "predictions" / "000123.label")
    got = np.fromfile(path, dtype=np.uint16)
    assert got.tolist() == list(output.KITTI_LEARNING_MAP_INV) + [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the offline tool
def test_map_sequence_tool_writes_mapped_frames_and_prints_both_blocks(monkeypatch, tmp_path, capsys):
    import pickle
    from occdepth_amd import fuse, output
    tool = _tool()
    KernelStandIn().install(monkeypatch)
    s = SampleStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    seq = _write_sequence(tmp_path / "08", "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 0.4\n1 0 0 0.2 0 1 0 0 0 0 1 1.0\n")
    frames = frames_for(dims, C, 21, 3, masked=True)
    pkl = tmp_path / "pkl"
    os.makedirs(pkl)
    for n, (lab, mask) in enumerate(frames):
        with open(pkl / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": lab.astype(np.uint16), "target": np.roll(lab, 1, axis=0).astype(np.uint16),
                         "fov_mask_1": mask.reshape(-1)}, f)
    base = ["--poses", seq, "--pred", str(pkl), "--gt", str(pkl), "--out", str(tmp_path / "m" / "08"), "--dims", "16", "12", "8",
            "--origin"] + [str(o) for o in origin] + ["--fov"]
    tool.run(tool.parser().parse_args(base), device=torch.device("cpu"))
    plain = capsys.readouterr().out
    assert "frames======" not in plain and "mapped======" not in plain and not s.calls      # existing output is unchanged
    out_dir = tmp_path / "frames"
    tool.run(tool.parser().parse_args(base + ["--frames-out", str(out_dir), "--exclude-self", "--keep-own"]), device=torch.device("cpu"))
    out = capsys.readouterr().out
    assert out.startswith(plain) and out.index("frames======") < out.index("mapped======") and out.count("mIoU=") == 3
    assert len(s.calls) == 3 and all(c["exclude_self"] and c["keep_own"] and c["mask"] for c in s.calls)
    poses = fuse.read_kitti_poses(seq)
    ref = MapRef(C, origin, dims)
    for n, (lab, mask) in enumerate(frames):
        ref.integrate(lab, poses[n], mask)
    ids = np.array(output.KITTI_LEARNING_MAP_INV + (0,) * 236, dtype=np.uint16)
    names = sorted(os.listdir(out_dir / "sequences" / "08" / "predictions"))
    assert names == ["%06d.label" % n for n in range(3)]                   # one file per frame
    for n, (lab, mask) in enumerate(frames):
        own = np.minimum(lab, 255)
        mapped, _ = sample_ref(ref, poses[n], own, mask, 1, True, True)
        got = np.fromfile(str(out_dir / "sequences" / "08" / "predictions" / names[n]), dtype=np.uint16)
        assert np.array_equal(got, ids[mapped.reshape(-1)])


# ------------------------------------------------------------------------------------------------ argument checks
def test_map_sample_entry_point_validates_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected
    host16 = np.zeros((2, 16), dtype=np.int32)

    def args():
        a = hip.MapSampleArgs()
        a.votes = a.table = a.cells = a.own = a.own_mask = a.labels = a.n_obs = ptr
        a.n_bricks, a.capacity, a.X, a.Y, a.Z, a.gx, a.gy, a.gz = 2, 4, 40, 24, 20, 4, 3, 3
        a.C, a.pitch, a.label_bytes, a.min_obs, a.flags = 20, 20, 1, 1, 3
        return a

    sample = hip_lib.occd_map_sample
    assert sample(None, None) == -1
    for field, value in (("votes", None), ("table", None), ("cells", None), ("labels", None), ("n_obs", None), ("C", 0), ("C", 33),
                         ("X", 0), ("Y", -1), ("Z", 0), ("gx", 0), ("gy", -2), ("gz", 0), ("n_bricks", 0), ("capacity", 0),
                         ("label_bytes", 0), ("label_bytes", 3), ("pitch", 19), ("pitch", 16), ("pitch", 22), ("pitch", 0),
                         ("votes", ptr + 2), ("min_obs", -1), ("flags", 4), ("flags", -1), ("own", None)):
        a = args()
        setattr(a, field, value)
        assert sample(ctypes.byref(a), None) == -1, (field, value)
    for flags in (1, 2):                                                   # either flag alone needs own as well
        a = args()
        a.own, a.flags = None, flags
        assert sample(ctypes.byref(a), None) == -1, flags
    a = args()
    a.X = a.Y = a.Z = 1 << 10                                              # 2^30 voxels
    assert sample(ctypes.byref(a), None) == -1
    a = args()
    a.gx = a.gy = a.gz = 1 << 10                                           # 2^30 cells
    assert sample(ctypes.byref(a), None) == -1
    for slot in (4, 1 << 20):                                              # a slot at or past the capacity
        a = args()
        host16[1, 0] = slot
        a.table_host = host16.ctypes.data
        assert sample(ctypes.byref(a), None) == -1, slot
    assert hip.ABI_VERSION == 22 and (hip.MAP_SAMPLE_EXCLUDE_SELF, hip.MAP_SAMPLE_KEEP_OWN) == (1, 2)
    assert ctypes.sizeof(hip.MapSampleArgs) == 8 * 8 + 25 * 4 + 4 and "occd_map_sample" in hip.EXPORTS
