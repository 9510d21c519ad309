"""GPU: the surface mesh kernels (K39, csrc/mesh.hip) against the restatement of tests/test_mesh.py, exactly."""
import numpy as np
import pytest
import torch

from occdepth_amd import hip, mesh
from test_mesh import B, assert_mesh_equal, mesh_ref, random_rows, window_case

pytestmark = pytest.mark.gpu


def run(rows, cells, cap=True):
    dev = torch.device("cuda")
    return hip.mesh_faces(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), torch.from_numpy(np.ascontiguousarray(cells)).to(dev),
                          cap_unknown=cap)


def check(rows, cells, cap=True):
    got, want = run(rows, cells, cap), mesh_ref(rows, cells, cap)
    assert_mesh_equal(got, want)
    return want


@pytest.mark.parametrize("cap", [True, False])
@pytest.mark.parametrize("density", [0.05, 0.5, 0.95])
def test_one_brick_of_random_labels(density, cap):
    rows = random_rows(1, density, seed=int(density * 100))
    assert {0, 255} <= set(rows.reshape(-1).tolist())
    want = check(rows, np.zeros((1, 1, 1), dtype=np.int32), cap)
    assert len(want[1]) > 0


@pytest.mark.parametrize("cap", [True, False])
def test_window_with_absent_bricks_borders_and_facing_pairs(cap):
    rows, cells = window_case()
    assert (cells >= 0).sum() == 10 and len(rows) == 11
    v, q, lab, d = check(rows, cells, cap)
    if cap:                                                                    # the two facing pairs give no face between them
        low = v[q][:, 0]
        for x, z in ((4, 4), (9, 9)):
            at = lambda y, code: ((low == (16 + x, y, z)).all(1) & (d == code)).any()
            assert not at(16, 3) and not at(16, 2) and at(15, 2) and at(17, 3)  # none on the shared plane, the far sides are there


def test_two_solid_bricks_have_faces_on_the_hull_only():
    rows = np.full((2, B ** 3), 6, dtype=np.uint8)
    cells = np.array([1, 0], dtype=np.int32).reshape(1, 2, 1)
    dev = torch.device("cuda")
    counts, _ = hip.mesh_count(torch.from_numpy(rows).to(dev), torch.from_numpy(cells).to(dev))
    assert counts.tolist() == [5 * B * B, 5 * B * B]
    v, q, lab, d = check(rows, cells)
    assert len(q) == 10 * B * B and len(v) == 2 * (17 * 33) + 2 * (17 * 33) + 2 * (17 * 17) - 4 * 33 - 4 * 17 - 4 * 17 + 8
    opened = run(rows, cells, cap=False)                                       # no observed free space anywhere
    assert [tuple(t.shape) for t in opened] == [(0, 3), (0, 4), (0,), (0,)]


def test_checkerboard_brick_has_the_largest_count():
    i, j, l = np.meshgrid(np.arange(B), np.arange(B), np.arange(B), indexing="ij")
    rows = np.where((i + j + l) % 2 == 0, 9, 0).astype(np.uint8).reshape(1, -1)
    v, q, lab, d = check(rows, np.zeros((1, 1, 1), dtype=np.int32))
    assert len(q) == 12288 and len(v) == 17 ** 3 - 4                           # four window corners touch a free voxel only


def test_a_volume_without_a_solid_voxel_stops_after_the_count(monkeypatch):
    calls = []
    emit = hip.mesh_emit
    monkeypatch.setattr(hip, "mesh_emit", lambda *a, **kw: (calls.append(1), emit(*a, **kw))[1])
    rows = np.zeros((2, B ** 3), dtype=np.uint8)
    rows[1, ::3] = 255
    got = run(rows, np.array([0, 1], dtype=np.int32).reshape(2, 1, 1))
    assert [tuple(t.shape) for t in got] == [(0, 3), (0, 4), (0,), (0,)] and not calls
    assert all(t.is_cuda for t in got) and [t.dtype for t in got] == [torch.int32, torch.int32, torch.uint8, torch.uint8]
    run(random_rows(1, 0.5, 1), np.zeros((1, 1, 1), dtype=np.int32))
    assert calls == [1]                                                        # the counter does see a call


def test_far_corners_of_a_wide_window_sort_in_two_stages():
    grid = (2048, 2048, 1)
    assert sum(hip.mesh_key_bits(grid)) == 37
    rows = random_rows(2, 0.4, seed=11)
    dev = torch.device("cuda")
    cells = torch.full(grid, -1, dtype=torch.int32, device=dev)
    cells[0, 0, 0], cells[2047, 2047, 0] = 1, 0
    got = hip.mesh_faces(torch.from_numpy(rows).to(dev), cells)
    # the restatement on the two bricks side by side with a gap (no shared plane), moved to their places
    small = np.array([1, -1, 0], dtype=np.int32).reshape(3, 1, 1)
    v, q, lab, d = mesh_ref(rows, small)
    shift = np.where(v[:, :1] >= 2 * B, np.array([[2045 * B, 2047 * B, 0]]), 0).astype(np.int32)
    assert (v[:, 0] <= B).any() and (v[:, 0] >= 2 * B).any() and not ((v[:, 0] > B) & (v[:, 0] < 2 * B)).any()
    assert_mesh_equal(got, (v + shift, q, lab, d))
    assert got[0].max(0).values.tolist() == [2048 * B, 2048 * B, B]            # x sits in key bits 21 .. 36


def test_mesh_labels_on_a_frame_that_is_no_multiple_of_the_brick():
    rng = np.random.default_rng(17)
    labels = rng.integers(0, 20, size=(40, 24, 20)).astype(np.uint8)
    labels[rng.random(labels.shape) < 0.5] = 0
    labels[rng.random(labels.shape) < 0.05] = 255
    m = mesh.mesh_labels(torch.from_numpy(labels).cuda(), 0.2, (0.0, -25.6, -2.0))
    padded = np.full((48, 32, 32), 255, dtype=np.uint8)
    padded[:40, :24, :20] = labels
    rows = padded.reshape(3, B, 2, B, 2, B).transpose(0, 2, 4, 1, 3, 5).reshape(-1, B ** 3)
    want = mesh_ref(rows, np.arange(12, dtype=np.int32).reshape(3, 2, 2))
    assert_mesh_equal((m.vertices, m.quads, m.face_label, m.face_dir), want)
    assert m.vertices.is_cuda and want[0].max(0).tolist() == [40, 24, 20]
    assert np.array_equal(m.world_vertices()[-1], (np.array([0.0, -25.6, -2.0]) / 0.2 + want[0][-1]) * 0.2)


def test_two_runs_give_the_same_bytes_and_the_ply_reads_back(tmp_path):
    rows, cells = window_case()
    first, second = run(rows, cells), run(rows, cells)
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    m = mesh.Mesh(*first, np.array([-32, 16, 0]), 0.2)
    colours = np.arange(72, dtype=np.uint8).reshape(24, 3)
    back = mesh.read_mesh_ply(mesh.write_mesh_ply(str(tmp_path / "w.ply"), m, colours))
    assert np.array_equal(back["vertices"], m.world_vertices().astype(np.float32)) and back["voxel_size"] == 0.2
    assert np.array_equal(back["faces"], first[1].cpu().numpy()) and np.array_equal(back["label"], first[2].cpu().numpy())
    assert np.array_equal(back["rgb"], colours[first[2].cpu().numpy()])
