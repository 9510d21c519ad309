"""GPU: occd_map_integrate_weighted and occd_map_sample_weighted against `WeightedMapRef` / `sample_ref_weighted`, the
integer restatements of tests/test_visibility.py.  Everything is integer arithmetic on both sides: every comparison is
exact equality over every counter and every voxel.

Grids (40, 24, 20) and (16, 12, 8), the six-frame sequence of tests/test_map.py, chunk_bricks = 8 (the pool regrows), C in
{20, 12}, labels of 1 and 2 bytes, random weights in 0..255 of which a third are 0."""
import functools

import numpy as np
import pytest
import torch

from occdepth_amd import semantic_map as sm
from test_map import GRIDS, V, assert_map_equals_ref, frames_for, pose, sequence
from test_map_sample import sample_ref
from test_visibility import WeightedMapRef, sample_ref_weighted, weighted_frames

pytestmark = pytest.mark.gpu

CASES = [((40, 24, 20), 20, 1), ((40, 24, 20), 12, 2), ((16, 12, 8), 20, 2), ((16, 12, 8), 12, 1)]
IDS = ["%dx%dx%d-C%d-b%d" % (d + (c, b)) for d, c, b in CASES]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]       # (exclude_self, keep_own)


def _tensor(a):
    return torch.from_numpy(a if a.dtype != np.uint16 else a.view(np.int16)).cuda()


def frames_of(case):
    dims, C, label_bytes = case
    return weighted_frames(dims, C, 100 * C + label_bytes, 6, label_bytes)


@functools.lru_cache(maxsize=None)
def built(case, which=tuple(range(6))):
    """(map on the GPU, restatement) after the frames `which` of the sequence; shared by the tests, never changed."""
    dims, C, _ = case
    m, ref = sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=8), WeightedMapRef(C, GRIDS[dims], dims)
    frames, poses = frames_of(case), sequence(dims)
    for i in which:
        m.integrate(_tensor(frames[i][0]), poses[i], weight=_tensor(frames[i][1]))
        ref.integrate(frames[i][0], poses[i], weight=frames[i][1])
    return m, ref


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weighted_integrate_equals_the_restatement(case):
    m, ref = built(case)
    assert m.grown >= 2 and max(int(v.max()) for v in ref.votes.values()) > 255       # the pool regrew; weights add up
    assert_map_equals_ref(m, ref)


@pytest.mark.parametrize("flags", FLAGS, ids=["plain", "exclude_self", "keep_own", "exclude_self-keep_own"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weighted_sample_equals_the_restatement(case, flags):
    m, ref = built(case)
    frames, poses = frames_of(case), sequence(case[0])
    for i, ((own, weight), P) in enumerate(zip(frames, poses)):
        # the weights it voted with; for the last frame others, so that counters below the weight are met too
        w = weight if i < 5 else frames[0][1]
        min_obs = (1, 200)[i % 2]                                            # vote units: 200 is less than one heavy vote
        got = m.sample(P, own=_tensor(own), own_weight=_tensor(w), min_obs=min_obs, exclude_self=flags[0], keep_own=flags[1])
        want = sample_ref_weighted(ref, P, own, w, min_obs, *flags)
        assert got[0].dtype == torch.uint8 and got[1].dtype == torch.int16
        assert np.array_equal(got[0].cpu().numpy(), want[0]), (min_obs, i)
        assert np.array_equal(got[1].cpu().numpy().view(np.uint16), want[1]), (min_obs, i)
        if flags[0] and i == 1:                                              # the flag does retract
            assert (sample_ref(ref, P, own, None, min_obs, False, flags[1])[1] != want[1]).any()


@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=[IDS[1], IDS[3]])
def test_weights_of_zero_and_one_are_the_mask(case):
    dims, C, label_bytes = case
    origin = GRIDS[dims]
    frames, poses = frames_for(dims, C, 7 * C + label_bytes, 6, label_bytes, masked=True), sequence(dims)
    weighted, plain = (sm.SemanticMap(C, V, origin, dims, chunk_bricks=8) for _ in range(2))
    for (lab, mask), P in zip(frames, poses):
        weighted.integrate(_tensor(lab), P, weight=torch.from_numpy(mask.astype(np.uint8)).cuda())
        plain.integrate(_tensor(lab), P, mask=torch.from_numpy(mask).cuda())
    assert weighted.directory == plain.directory and torch.equal(weighted.votes, plain.votes)      # the same pool bytes
    for (lab, mask), P in zip(frames, poses):
        for flags in FLAGS:
            a = weighted.sample(P, own=_tensor(lab), own_weight=torch.from_numpy(mask.astype(np.uint8)).cuda(), min_obs=2,
                                exclude_self=flags[0], keep_own=flags[1])
            b = plain.sample(P, own=_tensor(lab), own_mask=torch.from_numpy(mask).cuda(), min_obs=2, exclude_self=flags[0],
                             keep_own=flags[1])
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), flags


def test_saturation_and_the_retraction_rule():
    """Weight 255 on the small grid until counters reach 65535 (257 votes of 255 are 65535 exactly), beside voxels of
    weight 1 and weight 0: a saturated counter is not retracted, one below the weight is not, every other is."""
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    lab = frames_for(dims, C, 11, 1)[0][0]
    weight = np.full(dims, 255, dtype=np.uint8)
    weight[::2] = 1
    weight[:, ::3] = 0
    m, ref = sm.SemanticMap(C, V, origin, dims), WeightedMapRef(C, origin, dims)
    dev_lab, dev_w = _tensor(lab), _tensor(weight)
    for n in range(258):
        m.integrate(dev_lab, pose(), weight=dev_w)
        if n in (255, 256, 257):                                             # 65280, 65535 reached exactly, 65535 kept
            ref.votes, ref._bricks = {}, None
            ref.integrate(lab, pose(), weight=(weight.astype(np.int64) * (n + 1)))
            assert_map_equals_ref(m, ref)
    top = (m.votes.to(torch.int32) & 0xFFFF).max().item()
    assert top == 65535 and max(int(v.max()) for v in ref.votes.values()) == 258 * 255
    for own_w in (weight, np.full(dims, 255, dtype=np.uint8), np.full(dims, 3, dtype=np.uint8)):
        for flags in FLAGS:
            got = m.sample(pose(), own=dev_lab, own_weight=_tensor(own_w), min_obs=1, exclude_self=flags[0], keep_own=flags[1])
            want = sample_ref_weighted(ref, pose(), lab, own_w, 1, *flags)
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy().view(np.uint16), want[1])
    # spelled out on the counts: with the weights it voted with, 65535 stays and 258 becomes 257
    kept = sample_ref_weighted(ref, pose(), lab, weight, 1, False, False)[1]
    less = m.sample(pose(), own=dev_lab, own_weight=dev_w, exclude_self=True)[1].cpu().numpy().view(np.uint16)
    assert set(np.unique(kept).tolist()) == {0, 258, 65535} and set(np.unique(less).tolist()) <= {0, 257, 258, 65535}
    assert ((kept == 65535) == (less == 65535)).all() and (less == 257).any()
    # a weight of 255 asked back from a counter of 258 is taken, from one of 3 it would not be: 258 - 255 = 3
    big = m.sample(pose(), own=dev_lab, own_weight=_tensor(np.full(dims, 255, dtype=np.uint8)), exclude_self=True)[1]
    assert 3 in set(np.unique(big.cpu().numpy().view(np.uint16)).tolist())


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[IDS[0], IDS[3]])
def test_the_weighted_map_is_the_merge_of_the_maps_of_any_split(case):
    whole, ref = built(case)
    for split in (((0, 2, 4), (1, 3, 5)), ((0, 1), (2, 3), (4, 5))):
        parts = [built(case, which)[0] for which in split]
        dims, C, _ = case
        total = sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=8)
        for part in parts:
            total.merge(part)
        assert_map_equals_ref(total, ref)
        keys = whole.brick_keys()
        assert torch.equal(total.brick_labels(keys), whole.brick_labels(keys))
