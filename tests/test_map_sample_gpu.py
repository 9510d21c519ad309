"""GPU: occd_map_sample (K32) against `sample_ref`, the numpy int64 restatement of tests/test_map_sample.py.  The world
voxel, the self-exclusion and the decision are integer arithmetic on both sides, so every comparison is exact equality
over every voxel of both outputs: no tolerance, no exclusions.

The maps are those of tests/test_map_gpu.py: grids (40, 24, 20) and (16, 12, 8) (neither a multiple of the brick, world
zero inside the grid), the six-frame sequence, chunk_bricks = 8 (the pool has regrown), C in {20, 12} (pitch 20 / 12: a
partial last 8-byte piece), own as uint8 and as int16 bits, with and without a mask."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from occdepth_amd import semantic_map as sm
from test_map import GRIDS, V, MapRef, frames_for, pose, sequence
from test_map_gpu import CASES, IDS, _tensor, built
from test_map_sample import own_votes, sample_ref, world_voxels

pytestmark = pytest.mark.gpu

FLAGS = [(False, False), (True, False), (False, True), (True, True)]       # (exclude_self, keep_own)


def frames_of(case):
    dims, C, label_bytes, masked = case
    return frames_for(dims, C, 100 * C + label_bytes, 6, label_bytes, masked)      # the frames built() integrated


def away(dims):
    """A pose whose window meets no brick of the map, and one that meets only some."""
    return pose(5.2, 0.7, (60.0, 0.3, 0.1)), pose(9.0, 1.0, (dims[0] * V * 0.6, 0.2, 0.1))


def check(m, ref, P, own, mask, min_obs, flags):
    got = m.sample(P, own=None if own is None else _tensor(own), own_mask=None if mask is None else torch.from_numpy(mask).cuda(),
                   min_obs=min_obs, exclude_self=flags[0], keep_own=flags[1])
    want = sample_ref(ref, P, own, mask, min_obs, *flags)
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.int16 and tuple(got[0].shape) == tuple(got[1].shape) == ref.dims
    assert np.array_equal(got[0].cpu().numpy(), want[0]), (min_obs, flags)
    assert np.array_equal(got[1].cpu().numpy().view(np.uint16), want[1]), (min_obs, flags)
    return want


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "exclude_self", "keep_own", "exclude_self-keep_own"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sample_equals_the_restatement(case, flags):
    m, ref = built(*case)
    frames, poses = frames_of(case), sequence(case[0])
    assert m.grown >= 2
    changed = seen = 0
    for min_obs in (1, 2, 60000):
        for (own, mask), P in zip(frames, poses):
            labels, n_obs = check(m, ref, P, own, mask, min_obs, flags)
            if min_obs == 60000:
                assert np.array_equal(labels, np.minimum(own, 255).astype(np.uint8))       # nothing has that many votes
            changed += int((labels != np.minimum(own, 255)).sum())
            seen += int((n_obs > 1).sum())
        none, some = away(case[0])
        labels, n_obs = check(m, ref, none, frames[0][0], frames[0][1], min_obs, flags)
        assert not n_obs.any() and np.array_equal(labels, np.minimum(frames[0][0], 255).astype(np.uint8))
        labels, n_obs = check(m, ref, some, frames[1][0], frames[1][1], min_obs, flags)
        assert (n_obs == 0).any() and (n_obs > 0).any()
    assert changed > 0 and seen > 0                                        # the map does overrule frames, from several votes


@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_sample_without_own_gives_255_where_nothing_was_seen(case):
    m, ref = built(*case)
    for P in sequence(case[0])[:5] + list(away(case[0])):
        for min_obs in (1, 2):
            labels, n_obs = check(m, ref, P, None, None, min_obs, (False, False))
            assert (labels[n_obs < min_obs] == 255).all()
    assert (check(m, ref, away(case[0])[0], None, None, 1, (False, False))[0] == 255).all()


def test_the_tie_rule():
    dims, C = (16, 12, 8), 12
    origin = GRIDS[dims]
    m, ref = sm.SemanticMap(C, V, origin, dims), MapRef(C, origin, dims)
    for value in (7, 3, 11, 3, 7):                                         # 7 and 3 twice each, 11 once
        lab = np.full(dims, value, dtype=np.uint8)
        m.integrate(_tensor(lab), pose())
        ref.integrate(lab, pose())
    for own_class, flags, winner in ((7, (False, False), 3), (7, (False, True), 7), (11, (False, True), 3), (3, (False, True), 3),
                                     (255, (False, True), 3)):
        own = np.full(dims, own_class, dtype=np.uint8)
        labels, n_obs = check(m, ref, pose(), own, None, 1, flags)
        # (this lattice lies on the world-voxel boundaries: a frame voxel reads the world voxel its neighbour voted into,
        # and the last plane of every axis reads one nobody voted into)
        voted = n_obs == 5
        assert voted.sum() == 15 * 11 * 7 and not n_obs[~voted].any(), (own_class, flags)
        assert (labels[voted] == winner).all() and (labels[~voted] == own_class).all(), (own_class, flags)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_exclude_self_equals_the_map_of_the_other_frames(case):
    dims, C, label_bytes, masked = case
    origin = GRIDS[dims]
    frames, poses = frames_of(case), sequence(dims)
    whole = built(*case)[0]
    others = sm.SemanticMap(C, V, origin, dims, chunk_bricks=8)
    for i, ((lab, mask), P) in enumerate(zip(frames, poses)):
        if i != 3:
            others.integrate(_tensor(lab), P, mask=None if mask is None else torch.from_numpy(mask).cuda())
    assert int((whole.votes.to(torch.int32) & 0xFFFF).max()) < 65535       # no counter saturates at these sizes
    own, mask = frames[3]
    dev_mask = None if mask is None else torch.from_numpy(mask).cuda()
    for keep_own in (False, True):
        for min_obs in (1, 2):
            got = whole.sample(poses[3], own=_tensor(own), own_mask=dev_mask, min_obs=min_obs, exclude_self=True, keep_own=keep_own)
            want = others.sample(poses[3], own=_tensor(own), own_mask=dev_mask, min_obs=min_obs, keep_own=keep_own)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    kept = whole.sample(poses[3], own=_tensor(own), own_mask=dev_mask)
    assert bool((kept[1] != want[1]).any())                                # and without the flag the vote is there


def test_a_saturated_counter_is_not_retracted():
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    lab = frames_for(dims, C, 11, 1)[0][0]
    P = pose(17.3, 2.1, (1.13, -0.57, 0.21))
    m, ref = sm.SemanticMap(C, V, origin, dims), MapRef(C, origin, dims)
    m.integrate(_tensor(lab), P)
    ref.integrate(lab, P)
    # two frame voxels that read a world voxel holding this frame's vote and nothing else
    world = world_voxels(P, origin, dims)
    vote = own_votes(P, origin, dims, C, world, lab, None)
    picked = []
    for s in np.nonzero(vote >= 0)[0].tolist():
        w = tuple(world[s].tolist())
        if ref.votes[w].sum() == 1 and w not in [p[1] for p in picked]:
            picked.append((s, w, int(vote[s])))
        if len(picked) == 2:
            break
    for (s, w, c), (bits, value) in zip(picked, ((-1, 70000), (-2, 65534))):   # 65535 (the restatement counted on) and 65534
        slot = int(m.slots(np.array([[x // 16 for x in w]]))[0])
        m.votes[(slot,) + tuple(x % 16 for x in w) + (c,)] = bits
        ref.votes[w][c] = value
    ref._bricks = None
    n_obs = check(m, ref, P, lab, None, 1, (True, False))[1].reshape(-1)
    assert (int(n_obs[picked[0][0]]), int(n_obs[picked[1][0]])) == (65535, 65533)
    plain = check(m, ref, P, lab, None, 1, (False, False))[1].reshape(-1)
    assert (int(plain[picked[0][0]]), int(plain[picked[1][0]])) == (65535, 65534)


def test_model_hook_scores_the_mapped_frames_of_real_maps(tmp_path):
    from occdepth_amd import fuse, hip, output
    from occdepth_amd.models.OccDepth import OccDepth
    from test_map import HOOK_C, HOOK_DIMS, HOOK_ORIGIN, _hook_steps, _hook_stub, _write_sequence
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    sub = tmp_path / "sub"
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps"), str(root), frames=True,
                                        submission_dir=str(sub), exclude_self=True)
    steps = [(batch, logits.cuda(), target.cuda()) for batch, logits, target in _hook_steps()]
    for batch, logits, target in steps:
        OccDepth._map_step(stub, "val", batch, logits, target)
    assert all(t[0].is_cuda and t[1].is_cuda and t[2].is_cuda for v in stub.semantic_map["kept"].values() for t in v)
    assert OccDepth._map_epoch_end(stub, "val") is not None and stub.semantic_map["kept"] == {}
    want = np.zeros((HOOK_C, HOOK_C), dtype=np.int64)
    ids = np.array(output.KITTI_LEARNING_MAP_INV, dtype=np.uint16)
    for seq in ("03", "08"):
        poses = fuse.read_kitti_poses(str(root / seq))
        ref = MapRef(HOOK_C, HOOK_ORIGIN, HOOK_DIMS, 0.2)
        mine = [(hip.argmax_labels_u16(logits[i:i + 1])[0].cpu().numpy().astype(np.uint8), target[i].cpu().numpy(),
                 batch["fov_mask_1"][i].numpy(), poses[int(batch["frame_id"][i])], batch["frame_id"][i])
                for batch, logits, target in steps for i, q in enumerate(batch["sequence"]) if q == seq]
        for pred, _, mask, P, _ in mine:
            ref.integrate(pred, P, mask)
        for pred, target, mask, P, frame_id in mine:
            mapped, _ = sample_ref(ref, P, pred, mask, 1, True, True)
            keep = target != 255
            np.add.at(want, (target[keep].astype(np.int64), mapped[keep].astype(np.int64)), 1)
            data = np.fromfile(str(sub / "sequences" / seq / "predictions" / (frame_id + ".label")), dtype=np.uint16)
            assert np.array_equal(data, ids[mapped.reshape(-1)])
    assert want.sum() > 0 and np.array_equal(stub.hists[-2].cpu().numpy(), want)
    assert len(stub.semantic_map["mapped_stats"]["val"]["iou_ssc"]) == HOOK_C


@functools.lru_cache(maxsize=None)
def _bench():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bench_map_sample.py")
    spec = importlib.util.spec_from_file_location("bench_map_sample_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_torch_operator_formulation_gives_the_same_labels(case):
    bench = _bench()
    m, ref = built(*case)
    dims, C = case[0], case[1]
    dev = m.votes.device
    lattice = bench.frame_lattice(dims, dev)
    frames, poses = frames_of(case), sequence(dims)
    for (own, _), P in list(zip(frames, poses))[:5] + [(frames[1], away(dims)[1])]:
        cells, table, key_min = m.frame_cells(P, dev)
        Bq, dq = sm.sample_coefficients(P, m.vox_origin, m.voxel_size, key_min, dims)
        for min_obs, keep_own, use_own in ((1, True, True), (2, False, True), (1, False, False)):
            got = bench.torch_sample(m.pool(), torch.from_numpy(table).to(dev), torch.from_numpy(cells).to(dev),
                                     _tensor(own) if use_own else None, torch.from_numpy(Bq).to(dev), torch.from_numpy(dq).to(dev),
                                     lattice, C, min_obs, keep_own)
            want = m.sample(P, own=_tensor(own) if use_own else None, min_obs=min_obs, keep_own=keep_own)
            assert torch.equal(got[0], want[0].reshape(-1)) and torch.equal(got[1], want[1].reshape(-1)), (min_obs, keep_own)


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_sample_is_deterministic_and_leaves_the_pool_alone(case):
    m, _ = built(*case)
    (own, mask), P = frames_of(case)[4], sequence(case[0])[4]
    dev_mask = None if mask is None else torch.from_numpy(mask).cuda()
    before = m.votes.clone()
    state = (m.n_bricks, m.capacity, m.grown)
    a = m.sample(P, own=_tensor(own), own_mask=dev_mask, min_obs=2, exclude_self=True, keep_own=True)
    b = m.sample(P, own=_tensor(own), own_mask=dev_mask, min_obs=2, exclude_self=True, keep_own=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    m.sample(away(case[0])[1])
    assert torch.equal(m.votes, before) and (m.n_bricks, m.capacity, m.grown) == state
