"""GPU: occd_ccl_segments, occd_ccl_roots / occd_ccl_compact and occd_ccl_filter (K40) against the numpy restatements of
occdepth_amd/panoptic.py (tests/test_ccl.py pins those against a brute-force flood fill, scipy and hand cases).
Everything is an integer: every comparison is exact equality, on every element.

Shapes are the smallest at which each mechanism can still go wrong (T = the tile edge, 16): frames thinner than a tile,
tails on every axis, a path that crosses every seam many times, roots of whole tiles that change late, the largest number
of segments a volume can hold, and frames that must not leak into each other."""
import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd import panoptic as pan
from test_ccl import (STUFF, THINGS, T, checkerboard, comb, random_case, random_volume, serpentine, slabs, two_frames)

pytestmark = pytest.mark.gpu

RANDOM_SHAPES = ((1, 2 * T + 1, T + 1, T - 1), (1, 64, 48, 32))


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                          # a copy: the shared cases are read-only


def run(lab, things, stuff, connectivity, **kw):
    """-> seg, ids, count, (class, size, index) of the kernels, as numpy arrays."""
    dev = _dev(lab)
    seg = hip.ccl_segments(dev, things, stuff, connectivity, **kw)
    ids, count, offsets, tables = hip.ccl_compact(seg, dev)
    assert offsets.cpu().tolist() == (np.cumsum(count.numpy()) - count.numpy()).tolist()
    return (seg.cpu().numpy(), ids.cpu().numpy(), count.numpy()) + tuple(t.cpu().numpy() for t in tables)


def check(lab, things, stuff, connectivity, **kw):
    """Hold every output of the kernels to the restatement; -> the restatement's (seg, count, size)."""
    seg = pan.segments_ref(lab, things, stuff, connectivity)
    want = (seg,) + pan.compact_ref(seg, lab)
    got = run(lab, things, stuff, connectivity, **kw)
    for g, w, name in zip(got, want, ("seg", "ids", "count", "class", "size", "index")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), name
    return seg, want[2], want[4]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_degenerate_frames(connectivity):
    n = 2 * T + 3
    for shape in ((1, 1, 1, 1), (1, 1, 1, n), (1, n, 1, 1), (1, 1, n, 1)):
        solid = np.ones(shape, dtype=np.uint8)
        _, count, size = check(solid, (1,), (), connectivity)
        assert count.tolist() == [1] and size.tolist() == [solid.size]
        check(random_volume(shape, 0.7, seed=n), THINGS, STUFF, connectivity)
        check(np.zeros(shape, dtype=np.uint8), THINGS, STUFF, connectivity)
    lab = random_volume((1, 5, 4, 3), 0.5, seed=2)
    check(lab, (0, 1), (255,), connectivity)                            # the masks may name 0 and 255


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
@pytest.mark.parametrize("shape", RANDOM_SHAPES)
def test_random_volumes(shape, density, connectivity):
    c = random_case(shape, density, connectivity)
    got = run(c["labels"], THINGS, STUFF, connectivity)
    print(shape, density, connectivity, "segments", int(c["count"].sum()), "largest", int(c["size"].max()))
    assert c["count"].sum() > 2 and (c["labels"] == 255).any()
    for g, name in zip(got, ("seg", "ids", "count", "class", "size", "index")):
        assert g.dtype == c[name].dtype and np.array_equal(g, c[name]), name


@pytest.mark.parametrize("connectivity", [6, 26])
def test_two_calls_give_identical_bytes_and_the_tile_pass_changes_nothing(connectivity):
    c = random_case(RANDOM_SHAPES[0], 0.5, connectivity)
    dev = _dev(c["labels"])
    ws = hip.ccl_workspace(1, dev.shape[1:], dev.device)
    first = hip.ccl_segments(dev, THINGS, STUFF, connectivity, ws)
    again = hip.ccl_segments(dev, THINGS, STUFF, connectivity, ws)      # the workspace holds the first call's leftovers
    assert first.cpu().numpy().tobytes() == again.cpu().numpy().tobytes() == c["seg"].tobytes()
    untiled = hip.ccl_segments(dev, THINGS, STUFF, connectivity, ws, tile_pass=False)
    assert torch.equal(untiled, first)


def test_batch_of_random_frames():
    lab = random_volume((3, 2 * T + 1, T + 1, T - 1), 0.5, seed=11)
    _, count, _ = check(lab, THINGS, STUFF, 26)
    assert (count > 2).all()


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("gap", [False, True])
def test_serpentine(gap, connectivity):
    lab = serpentine(gap)
    _, count, size = check(lab, (1,), (), connectivity)
    assert count.tolist() == [2 if gap else 1] and size.sum() == (lab == 1).sum()
    check(lab, (1,), (), connectivity, tile_pass=False)                 # the chain at its longest: one union-find over it all


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("mirror", [False, True])
def test_comb(mirror, connectivity):
    _, count, _ = check(comb(mirror), (2,), (), connectivity)
    assert count.tolist() == [1]


def test_checkerboard_has_the_most_segments_under_6_and_one_under_26():
    lab = checkerboard()
    _, count, size = check(lab, (1,), (), 6)
    assert count.tolist() == [((T + 2) ** 3 + 1) // 2] and (size == 1).all()
    _, count, size = check(lab, (1,), (), 26)
    assert count.tolist() == [1]


@pytest.mark.parametrize("connectivity", [6, 26])
def test_neighbours_of_different_classes_never_merge(connectivity):
    lab = slabs()
    _, count, size = check(lab, (1, 2), (), connectivity)
    assert count.tolist() == [T + 3] and (size == (T + 1) * 5).all()


def test_solid_volume_is_one_component():
    lab = np.ones((1, 64, 64, 32), dtype=np.uint8)
    seg, ids, count, cls, size, index = run(lab, (1,), (), 26)
    assert (seg == 1).all() and (ids == 1).all() and count.tolist() == [1]
    assert cls.tolist() == [1] and size.tolist() == [2 ** 17] and index.tolist() == [0]
    seg6 = hip.ccl_segments(_dev(lab), (1,), (), 6)
    assert bool((seg6 == 1).all())


@pytest.mark.parametrize("second_empty", [False, True])
def test_nothing_leaks_across_frames(second_empty):
    lab = two_frames(second_empty)
    _, count, _ = check(lab, (1,), (9,), 26)
    assert count.tolist() == ([2, 0] if second_empty else [2, 2])


@pytest.mark.parametrize("shape", RANDOM_SHAPES)
@pytest.mark.parametrize("min_voxels", [1, 2, 5, 2 ** 31 - 1])
def test_filter(shape, min_voxels):
    changed = kept = False
    for density, connectivity in ((0.5, 26), (0.05, 6)):
        lab = random_case(shape, density, connectivity)["labels"]
        want = pan.filter_ref(lab, THINGS, min_voxels, connectivity)
        got = hip.ccl_filter(_dev(lab), THINGS, min_voxels, connectivity, STUFF).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        keep = ~np.isin(lab, THINGS)
        assert np.array_equal(got[keep], lab[keep])                     # stuff and every other label pass
        changed, kept = changed or bool((got != lab).any()), kept or bool(np.isin(got, THINGS).any())
    assert changed == (min_voxels > 1) and kept == (min_voxels < 2 ** 31 - 1)
    flat = pan.remove_small_components(_dev(lab[0]), min_voxels, THINGS, connectivity)
    assert flat.shape == lab.shape[1:] and np.array_equal(flat.cpu().numpy(), want[0])


def test_segments_by_instance_id():
    rng = np.random.default_rng(5)
    shape = (2, T + 3, 7, 5)
    lab = random_volume(shape, 0.6, seed=4)
    n = lab[0].size
    inst = rng.integers(-1, 40, size=shape).astype(np.int32)
    inst[0, 0, 0, :2] = (n, n - 1)                                       # n is out of range, n - 1 the largest id
    lab[0, 0, 0, :2] = 1
    inst[np.isin(lab, THINGS)] += 50 * lab[np.isin(lab, THINGS)].astype(np.int32)          # an id never spans two classes
    inst[0, 0, 0, :2] = (n, n - 1)
    inst[0, 1] = np.where(inst[0, 1] % 7 == 0, 0, inst[0, 1])           # ids <= 0 belong to no segment
    inst[0, 2, 0, 0] = -3
    want = pan.instance_segments_ref(lab, inst, THINGS, STUFF)
    got = hip.ccl_segments(_dev(lab), THINGS, STUFF, 26, instances=_dev(inst))
    assert np.array_equal(got.cpu().numpy(), want) and want[0, 0, 0, 0] == 0 and want[0, 0, 0, 1] == 2
    lab[1, 1, 1, 1], lab[1, 2, 2, 2] = 1, 2
    inst[1, 1, 1, 1] = inst[1, 2, 2, 2] = 7
    with pytest.raises(ValueError, match="more than one class"):
        hip.ccl_segments(_dev(lab), THINGS, STUFF, 26, instances=_dev(inst))
