"""CPU: the numpy restatements of occdepth_amd/panoptic.py (K40) -- segments_ref against a brute-force flood fill and
scipy.ndimage.label, hand cases, panoptic_ref on a hand-computed scene -- the argument checks of the occd_ccl_* entry
points, and the case builders tests/test_ccl_gpu.py and tests/test_panoptic_gpu.py hold the kernels to."""
import ctypes
import functools

import numpy as np
import pytest

from occdepth_amd import panoptic as pan

T = 16                                   # OCCD_CCL_TILE: the edge of the tile-local pass (test_tile_edge_is_the_headers pins it)
THINGS, STUFF = (1, 2, 3), (9, 10)


# ----------------------------------------------------------------------------------------------------- case builders
def random_volume(shape, density, seed):
    """uint8 (B, X, Y, Z): three things classes, two stuff classes, a class in neither set (5), free space and 255."""
    rng = np.random.default_rng(seed)
    lab = rng.choice(np.array([1, 2, 3, 9, 10, 5], dtype=np.uint8), size=shape, p=[0.3, 0.2, 0.2, 0.12, 0.12, 0.06])
    lab[rng.random(shape) >= density] = 0
    lab[rng.random(shape) < 0.02] = 255
    return lab


def serpentine_path(n, nz=4):
    """The voxels, in order, of a one-voxel-wide path through an n x n x nz volume: rows along x on every other y, joined at
    alternating ends, on the planes z = 0, 2, ..., joined through the planes between."""
    path, forward, up = [], True, True
    for z in range(0, nz, 2):
        rows = list(range(0, n, 2)) if up else list(range(0, n, 2))[::-1]
        for i, y in enumerate(rows):
            xs = list(range(n)) if forward else list(range(n))[::-1]
            path += [(x, y, z) for x in xs]
            if i + 1 < len(rows):
                path.append((xs[-1], (y + rows[i + 1]) // 2, z))
            forward = not forward
        if z + 2 < nz:
            path.append((path[-1][0], path[-1][1], z + 1))
        up = not up
    return path


def serpentine(gap):
    """(1, 2T + 2, 2T + 2, 4): one class along serpentine_path -- it crosses every tile seam many times; gap: the path's
    middle voxel (inside a row) is free, which cuts it in two."""
    n = 2 * T + 2
    path = serpentine_path(n)
    lab = np.zeros((1, n, n, 4), dtype=np.uint8)
    for x, y, z in path:
        lab[0, x, y, z] = 1
    if gap:
        x, y, z = path[len(path) // 2 + 5]
        assert 2 < x < n - 3                                            # inside a row: its two neighbours are two apart
        lab[0, x, y, z] = 0
    return lab


def comb(mirror):
    """(1, 2T + 3, 2T + 3, 3): three teeth along x, each in another row of tiles, joined by a spine at x = 0 only (the
    smallest index: every tooth learns its root through the spine); mirror: the spine at the last x."""
    n = 2 * T + 3
    lab = np.zeros((1, n, n, 3), dtype=np.uint8)
    for y in (1, T + 1, 2 * T + 1):
        lab[0, :, y, 1] = 2
    lab[0, 0, :, 1] = 2
    return np.ascontiguousarray(lab[:, ::-1]) if mirror else lab


def checkerboard():
    i, j, k = np.indices((T + 2,) * 3)
    return (((i + j + k) % 2) == 0).astype(np.uint8)[None]


def slabs():
    """Two things classes in alternating one-voxel slabs along x: neighbours of different classes never merge."""
    lab = np.zeros((1, T + 3, T + 1, 5), dtype=np.uint8)
    lab[0, 0::2] = 1
    lab[0, 1::2] = 2
    return lab


def two_frames(second_empty):
    """(2, 5, 4, 3): the last voxels of frame 0 and the first of frame 1 carry one class."""
    lab = np.zeros((2, 5, 4, 3), dtype=np.uint8)
    lab[0, 4, 3, 1:] = 1
    lab[0, 0, 0, 0] = 9
    if not second_empty:
        lab[1, 0, 0, :2] = 1
        lab[1, 2, 2, 2] = 9
    return lab


def hand_scene():
    """One frame, 12 x 12 x 2, SemanticKITTI sets (car = 1; road = 9 and parking = 10 stuff) -> (pred, target).
    car A: 4 voxels, found shifted by one (3 shared of 5: IoU 3/5); car B: 3 voxels, found shifted by one (2 shared of 4: IoU
    exactly 1/2, no match); a car of 2 voxels where the target is free; road: 10 voxels, 8 found (IoU 8/10); parking: 10
    voxels, 4 found (IoU 4/10: below the threshold)."""
    target = np.zeros((1, 12, 12, 2), dtype=np.uint8)
    pred = np.zeros_like(target)
    target[0, 0:4, 0, 0] = 1
    pred[0, 1:5, 0, 0] = 1
    target[0, 0:3, 4, 0] = 1
    pred[0, 1:4, 4, 0] = 1
    pred[0, 0:2, 8, 0] = 1
    target[0, 0:10, 10, 1] = 9
    pred[0, 0:8, 10, 1] = 9
    target[0, 0:10, 11, 0] = 10
    pred[0, 6:10, 11, 0] = 10
    return pred, target


HAND_SETS = (pan.KITTI_THINGS, pan.KITTI_STUFF)


@functools.lru_cache(maxsize=None)
def random_case(shape, density, connectivity):
    """-> the volume and the restatement's results on it, computed once and never written to."""
    lab = random_volume(shape, density, seed=sum(shape) + int(density * 100))
    seg = pan.segments_ref(lab, THINGS, STUFF, connectivity)
    ids, count, cls, size, index = pan.compact_ref(seg, lab)
    out = {"labels": lab, "seg": seg, "ids": ids, "count": count, "class": cls, "size": size, "index": index}
    for v in out.values():
        v.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------- segments_ref
def flood_fill(lab, things, stuff, connectivity):
    """Brute force: one stack-based fill per unvisited things voxel."""
    B, X, Y, Z = lab.shape
    seg = np.zeros(lab.shape, dtype=np.int32)
    nbrs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    for b in range(B):
        for x in range(X):
            for y in range(Y):
                for z in range(Z):
                    c = int(lab[b, x, y, z])
                    if c in stuff:
                        seg[b, x, y, z] = int(np.flatnonzero(lab[b].reshape(-1) == c)[0]) + 1
                    if c not in things or seg[b, x, y, z]:
                        continue
                    root, stack = (x * Y + y) * Z + z + 1, [(x, y, z)]
                    seg[b, x, y, z] = root
                    while stack:
                        i, j, k = stack.pop()
                        for dx, dy, dz in nbrs:
                            u, v, w = i + dx, j + dy, k + dz
                            if 0 <= u < X and 0 <= v < Y and 0 <= w < Z and lab[b, u, v, w] == c and not seg[b, u, v, w]:
                                seg[b, u, v, w] = root
                                stack.append((u, v, w))
    return seg


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("shape,density", [((2, 9, 7, 5), 0.5), ((1, 9, 7, 5), 0.95), ((1, 5, 1, 9), 0.6), ((1, 1, 1, 1), 1.0)])
def test_segments_ref_equals_flood_fill(shape, density, connectivity):
    lab = random_volume(shape, density, seed=sum(shape))
    assert np.array_equal(pan.segments_ref(lab, THINGS, STUFF, connectivity), flood_fill(lab, THINGS, STUFF, connectivity))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_segments_ref_equals_scipy_label(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    lab = random_volume((1, 21, 13, 10), 0.6, seed=3)
    got = pan.segments_ref(lab, THINGS, (), connectivity)[0]
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    want = np.zeros(lab.shape[1:], dtype=np.int64)
    for c in THINGS:
        comp, n = ndimage.label(lab[0] == c, structure=structure)
        flat = comp.reshape(-1)
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, flat, np.arange(flat.size))
        want = np.where(comp > 0, first[comp] + 1, want)                  # canonical form: 1 + the smallest index
    assert got.max() > 0 and np.array_equal(got, want)


def test_corner_contact_is_one_component_under_26_only():
    lab = np.zeros((1, 3, 3, 3), dtype=np.uint8)
    lab[0, 0, 0, 0] = lab[0, 1, 1, 1] = 1
    assert len(np.unique(pan.segments_ref(lab, (1,), (), 6))) == 3      # 0 and two segments
    seg = pan.segments_ref(lab, (1,), (), 26)
    assert seg[0, 0, 0, 0] == 1 and seg[0, 1, 1, 1] == 1 and len(np.unique(seg)) == 2


def test_empty_things_empty_stuff_and_unsegmented_labels():
    lab = random_volume((1, 6, 5, 4), 0.7, seed=1)
    assert (lab == 255).any() and (lab == 0).any() and (lab == 5).any()
    only_stuff = pan.segments_ref(lab, (), STUFF, 26)
    assert ((only_stuff != 0) == np.isin(lab, STUFF)).all()
    for c in STUFF:
        assert len(np.unique(only_stuff[lab == c])) == 1
    only_things = pan.segments_ref(lab, THINGS, (), 26)
    assert ((only_things != 0) == np.isin(lab, THINGS)).all()
    both = pan.segments_ref(lab, THINGS, STUFF, 26)
    assert (both[np.isin(lab, (0, 5, 255))] == 0).all() and (both[np.isin(lab, THINGS + STUFF)] > 0).all()
    with pytest.raises(ValueError):
        pan.segments_ref(lab, (1, 9), (9,), 26)


def test_case_builders_have_the_components_they_claim():
    def n_segments(lab, connectivity, things=(1, 2)):
        return int(pan.compact_ref(pan.segments_ref(lab, things, (), connectivity), lab)[1].sum())
    for connectivity in (6, 26):
        assert n_segments(serpentine(False), connectivity) == 1
        assert n_segments(serpentine(True), connectivity) == 2
        assert n_segments(comb(False), connectivity) == 1 and n_segments(comb(True), connectivity) == 1
        assert n_segments(slabs(), connectivity) == T + 3
    path = serpentine_path(2 * T + 2)
    assert len(set(path)) == len(path) and all(sum(abs(a - b) for a, b in zip(p, q)) == 1 for p, q in zip(path, path[1:]))
    assert n_segments(checkerboard(), 6) == ((T + 2) ** 3 + 1) // 2 and n_segments(checkerboard(), 26) == 1
    seg = pan.segments_ref(comb(True), (2,), (), 26)
    assert seg.max() == np.flatnonzero(comb(True).reshape(-1))[0] + 1
    a = pan.segments_ref(two_frames(False), (1,), (9,), 26)
    ids, count, cls, size, index = pan.compact_ref(a, two_frames(False))
    assert count.tolist() == [2, 2] and cls.tolist() == [9, 1, 1, 9] and size.tolist() == [1, 2, 2, 1]
    assert index.tolist() == [0, 58, 0, 32]
    assert pan.compact_ref(pan.segments_ref(two_frames(True), (1,), (9,), 26), two_frames(True))[1].tolist() == [2, 0]


def test_filter_ref_removes_small_things_only():
    lab = np.zeros((1, 6, 6, 2), dtype=np.uint8)
    lab[0, 0, 0, 0] = 1                     # one voxel
    lab[0, 2, 0:3, 0] = 1                   # three
    lab[0, 5, 5, 1] = 9                     # stuff, one voxel
    lab[0, 4, 0, 0] = 255
    assert np.array_equal(pan.filter_ref(lab, (1,), 1), lab)
    out = pan.filter_ref(lab, (1,), 2)
    assert out[0, 0, 0, 0] == 0 and (out[0, 2, 0:3, 0] == 1).all() and out[0, 5, 5, 1] == 9 and out[0, 4, 0, 0] == 255
    assert (pan.filter_ref(lab, (1,), 4) == 1).sum() == 0


# ----------------------------------------------------------------------------------------------------- panoptic_ref
def test_panoptic_ref_on_the_hand_scene():
    pred, target = hand_scene()
    counts, sums = pan.panoptic_ref(pred, target, 20, *HAND_SETS)
    for c, (tp, fp, fn) in {1: (1, 2, 1), 9: (1, 0, 0), 10: (0, 1, 1)}.items():
        assert (counts[pan.TP, c], counts[pan.FP, c], counts[pan.FN, c]) == (tp, fp, fn), c
    assert counts[:3].sum() == 7 and counts[pan.N_PRED].tolist()[1] == 3 and counts[pan.N_GT].tolist()[1] == 2
    assert sums[0, 1] == 3 / 5 and sums[0, 9] == 8 / 10 and sums[0, 10] == 0.0
    assert sums[1, 9] == 8 / 10 and sums[1, 10] == 4 / 10 and counts[pan.N_DAGGER].tolist()[9:11] == [1, 1]
    s = pan.panoptic_stats(counts, sums, *HAND_SETS)
    assert s["PQ_class"][1] == (3 / 5) / 2.5 and s["PQ_class"][9] == 0.8 and s["PQ_class"][10] == 0.0
    assert s["SQ_class"][1] == 3 / 5 and s["RQ_class"][1] == 1 / 2.5 and s["RQ_class"][9] == 1.0
    assert s["PQ"] == np.mean([(3 / 5) / 2.5, 0.8, 0.0]) and s["PQ_things"] == (3 / 5) / 2.5 and s["PQ_stuff"] == 0.4
    assert s["PQ_dagger"] == np.mean([(3 / 5) / 2.5, 0.8, 0.4])
    assert s["SQ"] == np.mean([3 / 5, 0.8, 0.0]) and s["RQ"] == np.mean([1 / 2.5, 1.0, 0.0])
    assert s["present"].tolist() == [c in (1, 9, 10) for c in range(20)]
    lines = pan.format_report(s, ["c%d" % i for i in range(20)], "test_pan")
    assert lines[0] == "test_pan======" and lines[1].startswith("PQ=34.6667, PQ_dagger=48.0000")


def test_strict_inequality_and_min_pred_voxels():
    pred, target = hand_scene()
    pred2 = pred.copy()
    pred2[0, 0, 4, 0] = 1                                               # car B now found with 3 shared of 4: IoU 3/4
    counts, sums = pan.panoptic_ref(pred2, target, 20, *HAND_SETS)
    assert (counts[pan.TP, 1], counts[pan.FP, 1], counts[pan.FN, 1]) == (2, 1, 0) and sums[0, 1] == 3 / 5 + 3 / 4
    counts, _ = pan.panoptic_ref(pred, target, 20, *HAND_SETS, min_pred_voxels=3)        # the 2-voxel car goes
    assert (counts[pan.TP, 1], counts[pan.FP, 1], counts[pan.FN, 1]) == (1, 1, 1)


def test_void_rule_and_mask():
    pred, target = hand_scene()
    base, _ = pan.panoptic_ref(pred, target, 20, *HAND_SETS)
    target2, pred2 = target.copy(), pred.copy()
    target2[0, 6:9, 6, 0] = 255
    pred2[0, 6:9, 6, 0] = 1                                             # a predicted car wholly in unknown voxels
    counts, _ = pan.panoptic_ref(pred2, target2, 20, *HAND_SETS)
    assert np.array_equal(counts, base)
    mask = np.ones(pred.shape, dtype=bool)
    mask[0, 0:2, 8, 0] = False                                          # the hallucinated car is masked out
    counts, _ = pan.panoptic_ref(pred, target, 20, *HAND_SETS, mask=mask)
    assert counts[pan.FP, 1] == base[pan.FP, 1] - 1 and counts[pan.TP, 1] == base[pan.TP, 1]


def test_target_instances_replace_the_components():
    pred, target = hand_scene()
    inst = np.zeros(target.shape, dtype=np.int32)
    inst[0, 0:4, 0, 0] = 7
    inst[0, 0:3, 4, 0] = 7                                              # both target cars are ONE annotated instance
    counts, sums = pan.panoptic_ref(pred, target, 20, *HAND_SETS, target_instances=inst)
    assert counts[pan.N_GT, 1] == 1 and counts[pan.TP, 1] == 0 and counts[pan.FP, 1] == 3 and counts[pan.FN, 1] == 1
    inst[0, 0, 10, 1] = 7                                               # a stuff voxel's id is ignored
    assert np.array_equal(pan.panoptic_ref(pred, target, 20, *HAND_SETS, target_instances=inst)[0], counts)
    target[0, 5, 5, 0], inst[0, 5, 5, 0] = 2, 7
    with pytest.raises(ValueError):
        pan.panoptic_ref(pred, target, 20, *HAND_SETS, target_instances=inst)


def test_overlaps_ref_rows():
    pred, target = hand_scene()
    g = pan.compact_ref(pan.segments_ref(target, *HAND_SETS), target)
    p = pan.compact_ref(pan.segments_ref(pred, *HAND_SETS), pred)
    rows = pan.overlaps_ref(g[0], g[1], p[0], p[1], target)
    assert rows[:, 2].sum() == ((pred != 0) | (target != 0)).sum()
    assert [tuple(r) for r in rows.tolist()] == sorted(tuple(r) for r in rows.tolist())
    car_a = [r for r in rows.tolist() if r[0] == 1]
    # the prediction's segments in index order: the car at (0, 8, 0), the road from (0, 10, 1), then the shifted car A
    assert car_a == [[1, 0, 1], [1, 3, 3]]                              # one voxel unmatched, three under the shifted car


# ----------------------------------------------------------------------------------------------------- the C entry points
def test_tile_edge_is_the_headers():
    from occdepth_amd import hip
    assert hip.CCL_TILE == T


def _valid_args(hip):
    buf = (ctypes.c_int64 * 4)()
    ptr = ctypes.addressof(buf)
    a = hip.CclArgs()
    for name in ("labels", "parent", "stuff_min", "status", "seg", "marks", "ranks", "offsets", "ids", "seg_class", "seg_size",
                 "seg_index", "out"):
        setattr(a, name, ptr)
    a.batch, a.X, a.Y, a.Z, a.connectivity, a.min_voxels, a.n_segments = 1, 4, 4, 4, 26, 1, 1
    a.things[0], a.stuff[0] = 0b0110, 0b1000
    return a, buf


def test_entry_points_validate_arguments_without_gpu(hip_lib):
    """Every OCCD_EINVAL case of the header, before any launch (no GPU is touched: each call has one invalid argument)."""
    from occdepth_amd import hip
    entries = (hip_lib.occd_ccl_segments, hip_lib.occd_ccl_roots, hip_lib.occd_ccl_compact, hip_lib.occd_ccl_filter)
    for fn in entries:
        assert fn(None, None) == -1
    for name, fns in (("labels", (0, 3)), ("parent", (0, 3)), ("stuff_min", (0,)), ("status", (0,)), ("seg", (0, 1, 2, 3)),
                      ("marks", (1,)), ("ranks", (2,)), ("offsets", (2,)), ("ids", (2,)), ("seg_class", (2,)), ("out", (3,))):
        a, buf = _valid_args(hip)
        setattr(a, name, None)
        for i in fns:
            assert entries[i](ctypes.byref(a), None) == -1, (name, i)
    for field, value in (("X", 0), ("Y", -1), ("Z", 0), ("batch", 0)):
        a, buf = _valid_args(hip)
        setattr(a, field, value)
        for fn in entries:
            assert fn(ctypes.byref(a), None) == -1, field
    a, buf = _valid_args(hip)
    a.X, a.Y, a.Z = 2048, 1024, 1024                                    # 2^31 voxels
    for fn in entries:
        assert fn(ctypes.byref(a), None) == -1
    a.X, a.Y, a.Z = 2 ** 31 - 1, 1, 1                                   # 2^31 - 1: one too many
    assert hip_lib.occd_ccl_segments(ctypes.byref(a), None) == -1
    for connectivity in (0, 18, 27):
        a, buf = _valid_args(hip)
        a.connectivity = connectivity
        assert hip_lib.occd_ccl_segments(ctypes.byref(a), None) == -1
    a, buf = _valid_args(hip)
    a.stuff[0] |= 0b0100                                                # class 2 in both masks
    assert hip_lib.occd_ccl_segments(ctypes.byref(a), None) == -1 and hip_lib.occd_ccl_filter(ctypes.byref(a), None) == -1
    for min_voxels in (0, -5):
        a, buf = _valid_args(hip)
        a.min_voxels = min_voxels
        assert hip_lib.occd_ccl_filter(ctypes.byref(a), None) == -1
    a, buf = _valid_args(hip)
    a.n_segments = -1
    assert hip_lib.occd_ccl_compact(ctypes.byref(a), None) == -1


def test_pair_entry_points_validate_arguments_without_gpu(hip_lib):
    from occdepth_amd import hip
    entries = (hip_lib.occd_ccl_pair_marks, hip_lib.occd_ccl_pair_emit, hip_lib.occd_ccl_pair_heads, hip_lib.occd_ccl_pair_rows)
    buf = (ctypes.c_int64 * 4)()

    def valid():
        a = hip.CclPairArgs()
        for name in ("g_ids", "p_ids", "target", "g_offsets", "p_offsets", "marks", "pos", "keys_lo", "refs", "ranks", "row_start",
                     "row_g", "row_p", "row_n"):
            setattr(a, name, ctypes.addressof(buf))
        a.n, a.batch, a.p_bits, a.n_pairs, a.n_rows = 64, 1, 4, 8, 2
        return a
    for fn in entries:
        assert fn(None, None) == -1
    for name, fns in (("g_ids", (0, 1)), ("p_ids", (0, 1)), ("target", (0, 1)), ("marks", (0, 2)), ("pos", (1,)), ("g_offsets", (1,)),
                      ("keys_lo", (1, 2, 3)), ("refs", (1,)), ("ranks", (3,)), ("row_start", (3,)), ("row_n", (3,))):
        a = valid()
        setattr(a, name, None)
        for i in fns:
            assert entries[i](ctypes.byref(a), None) == -1, (name, i)
    for field, value, fns in (("n", 0, (0, 1, 2, 3)), ("batch", 0, (0, 1, 2, 3)), ("n", 2 ** 31, (0, 1, 2, 3)), ("p_bits", 0, (0, 1, 2, 3)),
                              ("p_bits", 32, (0, 1, 2, 3)), ("n_pairs", 0, (1, 2, 3)), ("n_pairs", 65, (1, 2, 3)), ("n_rows", 0, (3,)),
                              ("n_rows", 9, (3,))):
        a = valid()
        setattr(a, field, value)
        for i in fns:
            assert entries[i](ctypes.byref(a), None) == -1, (field, value, i)
    a = valid()
    a.batch, a.n = 4, 2 ** 29                                           # 2^31 voxels in the batch
    assert hip_lib.occd_ccl_pair_marks(ctypes.byref(a), None) == -1


def test_off_means_nothing_is_imported():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; import occdepth_amd, occdepth_amd.models.OccDepth; "
            "assert 'occdepth_amd.panoptic' not in sys.modules, 'panoptic.py was imported with the switch off'")
    env = {k: v for k, v in os.environ.items() if not k.startswith("OCCDEPTH_PANOPTIC")}
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root, env=env)


def test_panoptic_metrics_are_switched_by_the_environment(monkeypatch):
    import golden_cases as gc
    import torch
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def state():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg).panoptic_metrics

    for var in ("OCCDEPTH_PANOPTIC", "OCCDEPTH_PANOPTIC_MIN_VOXELS", "OCCDEPTH_PANOPTIC_CONNECTIVITY", "OCCDEPTH_PANOPTIC_FOV",
                "OCCDEPTH_DIST_METRIC", "OCCDEPTH_RAY_METRIC", "OCCDEPTH_FUSE", "OCCDEPTH_MAP_DIR"):
        monkeypatch.delenv(var, raising=False)
    assert state() is None
    monkeypatch.setenv("OCCDEPTH_PANOPTIC_MIN_VOXELS", "4")              # without the switch: nothing
    assert state() is None
    monkeypatch.setenv("OCCDEPTH_PANOPTIC", "1")
    st = state()
    assert (st["connectivity"], st["min_pred_voxels"], st["fov_only"]) == (26, 4, False)
    assert (st["things"], st["stuff"]) == (pan.KITTI_THINGS, pan.KITTI_STUFF) and st["metrics"] == {} and st["fused"] == {}
    monkeypatch.setenv("OCCDEPTH_PANOPTIC_CONNECTIVITY", "6")
    assert state()["connectivity"] == 6
    monkeypatch.setenv("OCCDEPTH_PANOPTIC_CONNECTIVITY", "18")
    with pytest.raises(ValueError, match="connectivity"):
        state()
    monkeypatch.setenv("OCCDEPTH_PANOPTIC_CONNECTIVITY", "x")
    with pytest.raises(ValueError, match="OCCDEPTH_PANOPTIC"):
        state()


def test_python_wrappers_refuse_bad_arguments_without_gpu():
    import torch
    from occdepth_amd import hip
    lab = torch.zeros((1, 2, 2, 2), dtype=torch.uint8)
    with pytest.raises(ValueError):
        hip.ccl_segments(lab, (1,), (), connectivity=18)
    with pytest.raises(ValueError):
        hip.ccl_segments(lab, (1, 2), (2,))
    with pytest.raises(ValueError):
        hip.ccl_filter(lab, (1,), 0)
    with pytest.raises(RuntimeError):
        hip.ccl_segments(lab.to(torch.int32), (1,))
    with pytest.raises(RuntimeError):
        hip.ccl_segments(lab, (1,))                                     # a CPU tensor: there is no CPU path
    assert hip.ccl_class_mask((0, 31, 32, 255)) == (0x80000001, 1, 0, 0, 0, 0, 0, 0x80000000)
    with pytest.raises(ValueError):
        pan.PanopticMetrics(20, (1, 2), (2, 3))
    with pytest.raises(ValueError):
        pan.PanopticMetrics(20, (1,), (25,))
    m = pan.PanopticMetrics(20, *HAND_SETS)
    assert m.counts().shape == (6, 20) and m.counts().sum() == 0 and m.get_stats()["PQ"] == 0.0
    assert pan.default_classes("kitti") == (tuple(range(1, 9)), tuple(range(9, 20)))
    assert pan.default_classes("NYU") == (tuple(range(5, 12)), tuple(range(1, 5)))
