"""GPU: occd_map_integrate, occd_map_brick_labels, occd_map_count and occd_map_extract against `MapRef`, the numpy int64
restatement of tests/test_map.py.  Index selection is integer arithmetic on both sides, so every comparison is exact
equality over every voxel: no tolerance, no exclusions.

Grids (40, 24, 20) and (16, 12, 8): neither a multiple of the 16-voxel brick in every axis, origins that put world zero
inside the grid (negative keys).  Six frames: identity, an integer shift, a 90 degree yaw, two generic yaw + pitch
motions and a jump of more than a grid length, which brings only new bricks; chunk_bricks = 8 makes the pool regrow
between launches."""
import functools

import numpy as np
import pytest
import torch

from occdepth_amd import semantic_map as sm
from test_map import B, GRIDS, V, MapRef, assert_map_equals_ref, confusion_ref, frames_for, pose, sequence

pytestmark = pytest.mark.gpu

CASES = [((40, 24, 20), 20, 1, False), ((40, 24, 20), 12, 2, True), ((16, 12, 8), 20, 2, False), ((16, 12, 8), 12, 1, True)]
IDS = ["%dx%dx%d-C%d-b%d-%s" % (d + (c, b, "mask" if m else "whole")) for d, c, b, m in CASES]


def _tensor(lab):
    """uint8 stays uint8; uint16 values travel as the int16 tensor holding their bits."""
    return torch.from_numpy(lab if lab.dtype == np.uint8 else lab.view(np.int16)).cuda()


@functools.lru_cache(maxsize=None)
def built(dims, C, label_bytes, masked, n_frames=6):
    """(map on the GPU, restatement) after the first n_frames of the sequence; shared by the tests, never changed."""
    origin = GRIDS[dims]
    m = sm.SemanticMap(C, V, origin, dims, chunk_bricks=8)
    ref = MapRef(C, origin, dims)
    for (lab, mask), P in zip(frames_for(dims, C, 100 * C + label_bytes, n_frames, label_bytes, masked), sequence(dims)):
        m.integrate(_tensor(lab), P, mask=None if mask is None else torch.from_numpy(mask).cuda())
        ref.integrate(lab, P, mask)
    return m, ref


@functools.lru_cache(maxsize=None)
def ref_extract(case, min_obs, include_empty):
    return built(*case)[1].extract(min_obs, include_empty)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integrate_votes_equal_the_restatement(case):
    m, ref = built(*case)
    assert m.grown >= 2 and m.capacity % 8 == 0                            # the pool regrew between launches
    assert any(min(k) < 0 for k in ref.bricks()) and max(int(v.max()) for v in ref.votes.values()) >= 3
    assert_map_equals_ref(m, ref)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_brick_labels_equal_the_restatement(case):
    m, ref = built(*case)
    keys = m.brick_keys()
    missing = keys.max(0) + 1                                              # past every brick of the map
    lab = m.brick_labels(np.concatenate([keys, missing[None]])).cpu().numpy()
    assert lab.shape == (len(keys) + 1, B, B, B) and lab.dtype == np.uint8
    for i, k in enumerate(keys):
        assert np.array_equal(lab[i], ref.labels(k)), k
    assert (lab[-1] == 255).all() and (lab[:-1] != 255).any() and (lab[:-1] == 255).any()


def test_a_tie_goes_to_the_lowest_class():
    dims, C = (16, 12, 8), 12
    origin = GRIDS[dims]
    m, ref = sm.SemanticMap(C, V, origin, dims), MapRef(C, origin, dims)
    for value in (7, 3, 11, 3, 7):                                         # 7 and 3 twice each, 11 once: 3 wins
        lab = np.full(dims, value, dtype=np.uint8)
        lab[0] = 255 if value == 11 else value                             # and a plane where 11 never votes
        m.integrate(_tensor(lab), pose())
        ref.integrate(lab, pose())
    keys = m.brick_keys()
    got = m.brick_labels(keys).cpu().numpy()
    assert all(np.array_equal(got[i], ref.labels(k)) for i, k in enumerate(keys))
    assert sorted(set(got.reshape(-1).tolist())) == [3, 255]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_extract_equals_the_restatement_in_content_and_order(case):
    m = built(*case)[0]
    for min_obs, empty in ((1, False), (2, False), (1, True), (2, True), (60000, True)):
        want = ref_extract(case, min_obs, empty)
        got = m.extract(min_obs, empty)
        again = m.extract(min_obs, empty)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int16
        assert np.array_equal(got[0].cpu().numpy(), want[0]), (min_obs, empty)
        assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(got[2].cpu().numpy().view(np.uint16), want[2])
        assert all(torch.equal(a, b) for a, b in zip(got, again))          # bit-identical from run to run
        assert (len(want[1]) == 0) == (min_obs == 60000) and got[0].shape == (len(want[1]), 3)
    assert len(ref_extract(case, 1, True)[1]) > len(ref_extract(case, 1, False)[1]) > len(ref_extract(case, 2, False)[1]) > 0


def test_counters_saturate_at_65535():
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    lab = frames_for(dims, C, 11, 1)[0][0]
    m, ref = sm.SemanticMap(C, V, origin, dims), MapRef(C, origin, dims)
    m.integrate(_tensor(lab), pose())
    ref.integrate(lab, pose())
    w, vec = next((w, v) for w, v in sorted(ref.votes.items()) if min(w) < 0)
    c = int(vec.argmax())
    key, local = tuple(x // B for x in w), tuple(x % B for x in w)
    slot = int(m.slots(np.array([key]))[0])
    assert int(m.votes[(slot,) + local + (c,)]) == 1
    m.votes[(slot,) + local + (c,)] = -2                                   # the int16 that holds 65534
    for _ in range(3):
        m.integrate(_tensor(lab), pose())
        ref.integrate(lab, pose())
    ref.votes[w][c] = 65534 + 3                                            # the restatement counts on; the comparison clamps
    assert_map_equals_ref(m, ref)
    assert int(m.votes[(slot,) + local + (c,)]) == -1                      # 65535
    coords, labels, n_obs = m.extract(min_obs=5, include_empty=True)       # every other voxel has 4 votes
    assert coords.cpu().tolist() == [list(w)] and labels.cpu().tolist() == [c] and n_obs.cpu().tolist() == [-1]


def test_map_confusion_end_to_end():
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    dims, C = (16, 12, 8), 12
    pred, pred_ref = built(dims, C, 1, True)                               # six frames inside their masks
    gt, gt_ref = built(dims, C, 2, False, 5)                               # five whole frames, other labels
    want = confusion_ref(pred_ref, gt_ref, C)
    assert 0 < want.sum() < sum(1 for v in gt_ref.votes.values() if v.sum() > 0)
    for chunk in (512, 5):
        metric = sm.map_confusion(pred, gt, SSCMetrics(C), chunk_bricks=chunk)
        assert np.array_equal(metric.hist.cpu().numpy(), want)
