"""CPU: the surface mesh (K39, occdepth_amd/mesh.py) -- the restatement `mesh_ref` and checks that it is not its own
yardstick, the argument checks of the real library, the model hook and the two tools on a stand-in for the kernels, the PLY."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from occdepth_amd import hip, mesh
from occdepth_amd import semantic_map as sm
from test_map import (GRIDS, HOOK_C, KernelStandIn, _confusion_stand_in, _epoch, _hook_steps, _hook_stub, _tool,
                      _write_sequence, frames_for)
from test_map_render import densify

B = 16
# corner offsets of each face code, counter-clockwise seen from outside, from the lexicographically smallest corner
CORNERS = np.array([[(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],      # 0: -x
                    [(1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)],      # 1: +x
                    [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)],      # 2: -y
                    [(0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)],      # 3: +y
                    [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],      # 4: -z
                    [(0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]], dtype=np.int64)
NORMALS = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], dtype=np.int64)


def neighbour_labels(dense):
    """(6, X, Y, Z): the label next to every voxel towards each face code, 255 outside the window."""
    pad = np.pad(dense, 1, constant_values=255)
    X, Y, Z = dense.shape
    out = np.empty((6, X, Y, Z), dtype=np.uint8)
    for d, n in enumerate(NORMALS):
        out[d] = pad[1 + n[0]:1 + n[0] + X, 1 + n[1]:1 + n[1] + Y, 1 + n[2]:1 + n[2] + Z]
    return out


def mesh_ref(rows, cells, cap_unknown=True):
    """The contract restated by brute force on the dense window -> (vertices (V, 3), quads (F, 4), face_label, face_dir)."""
    rows, cells = np.asarray(rows).reshape(-1, B ** 3), np.asarray(cells)
    dense = densify(rows, np.where(cells < len(rows), cells, -1))
    solid = (dense >= 1) & (dense <= 254)
    nb = neighbour_labels(dense)
    exposed = solid[None] & ((nb == 0) | ((nb == 255) & bool(cap_unknown)))
    d, x, y, z = np.nonzero(exposed)
    row = cells[x // B, y // B, z // B].astype(np.int64)
    local = ((x % B) * B + (y % B)) * B + (z % B)
    order = np.lexsort((d, local, row))
    d, x, y, z = d[order], x[order], y[order], z[order]
    corners = np.stack([x, y, z], -1)[:, None, :] + CORNERS[d]                 # (F, 4, 3)
    dims = np.array(dense.shape, dtype=np.int64) + 1
    keys = (corners[..., 0] * dims[1] + corners[..., 1]) * dims[2] + corners[..., 2]
    uniq, inverse = np.unique(keys.reshape(-1), return_inverse=True)
    vertices = np.stack([uniq // (dims[1] * dims[2]), uniq // dims[2] % dims[1], uniq % dims[2]], -1).astype(np.int32)
    return vertices, inverse.reshape(-1, 4).astype(np.int32), dense[x, y, z], d.astype(np.uint8)


def assert_mesh_equal(got, want):
    for have, ref, name in zip(got, want, ("vertices", "quads", "face_label", "face_dir")):
        have = have.cpu().numpy() if torch.is_tensor(have) else np.asarray(have)
        assert have.shape == ref.shape and have.dtype == ref.dtype and np.array_equal(have, ref), name


def random_rows(n, density, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(1, 20, size=(n, B ** 3)).astype(np.uint8)
    u = rng.random((n, B ** 3))
    lab[u >= density] = 0
    lab[rng.random((n, B ** 3)) < 0.1] = 255
    return lab


def window_case(seed=3):
    """The 3 x 3 x 2 window of the GPU tests: absent bricks, a row no cell points to, solid voxels on every border plane of
    a brick and at the window's outer faces, solid pairs across a brick border of equal and of different class."""
    rng = np.random.default_rng(seed)
    cells = np.full((3, 3, 2), -1, dtype=np.int32)
    at = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (0, 2, 1), (2, 2, 0), (1, 2, 1), (2, 0, 1), (1, 0, 1)]
    rows = random_rows(len(at) + 1, 0.3, seed)
    order = rng.permutation(len(at) + 1)                                       # rows in no spatial order; one stays unused
    for c, r in zip(at, order[:len(at)]):
        cells[c] = r
    centre = rows[cells[1, 1, 0]].reshape(B, B, B)
    for plane in (centre[0], centre[-1], centre[:, 0], centre[:, -1], centre[:, :, 0], centre[:, :, -1]):
        plane[2:6, 3:9] = 7
    a, b = rows[cells[1, 0, 0]].reshape(B, B, B), rows[cells[1, 1, 0]].reshape(B, B, B)
    a[4, 15, 4], b[4, 0, 4] = 5, 5                                             # equal class across the y border
    a[9, 15, 9], b[9, 0, 9] = 5, 11                                            # different class
    a[4, 14, 4] = a[9, 14, 9] = b[4, 1, 4] = b[9, 1, 9] = 0                    # their far sides face free space
    rows[cells[0, 0, 0]].reshape(B, B, B)[0, :4, :4] = 3                       # at the window's outer faces
    rows[cells[2, 2, 0]].reshape(B, B, B)[15, 12:, 0] = 9
    rows[order[-1]] = 13                                                       # present in labels, -1 in cells: never meshed
    return rows, cells


def edge_use(quads):
    e = np.stack([quads, np.roll(quads, -1, axis=1)], -1).reshape(-1, 2)
    _, counts = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    return counts


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_single_voxel():
    rows = np.zeros((1, B ** 3), dtype=np.uint8)
    rows[0, (5 * B + 6) * B + 7] = 4
    v, q, lab, d = mesh_ref(rows, np.zeros((1, 1, 1), dtype=np.int32))
    assert len(v) == 8 and len(q) == 6 and d.tolist() == [0, 1, 2, 3, 4, 5] and set(lab.tolist()) == {4}
    assert v.min(0).tolist() == [5, 6, 7] and v.max(0).tolist() == [6, 7, 8]
    assert np.array_equal(v, v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))])


@pytest.mark.parametrize("cap", [True, False])
def test_normals_edges_and_divergence(cap):
    rows, cells = window_case()
    v, q, lab, d = mesh_ref(rows, cells, cap)
    p = v[q].astype(np.int64)
    assert np.array_equal(np.cross(p[:, 1] - p[:, 0], p[:, 3] - p[:, 0]), NORMALS[d])
    assert np.array_equal(p[:, 2] - p[:, 0], (p[:, 1] - p[:, 0]) + (p[:, 3] - p[:, 0]))
    assert (p[:, 0][:, None, :] <= p).all()                                    # the smallest corner comes first
    assert len(np.unique(v, axis=0)) == len(v) and set(np.unique(q).tolist()) == set(range(len(v)))
    if not cap:
        return
    assert (edge_use(q) % 2 == 0).all()
    dense = densify(rows, cells)
    n_solid = int(((dense >= 1) & (dense <= 254)).sum())
    for axis in range(3):
        plus, minus = d == 2 * axis + 1, d == 2 * axis
        assert int(p[plus, 0, axis].sum()) - int(p[minus, 0, axis].sum()) == n_solid


def test_open_mesh_is_the_subset_towards_free_space():
    rows, cells = window_case()
    closed, opened = mesh_ref(rows, cells, True), mesh_ref(rows, cells, False)
    nb = neighbour_labels(densify(rows, cells))
    vc = closed[0][closed[1]]                                                  # (F, 4, 3) corner coordinates
    voxel = vc[:, 0] - np.maximum(NORMALS[closed[3]], 0)                       # the smallest corner back to the voxel
    free = nb[closed[3], voxel[:, 0], voxel[:, 1], voxel[:, 2]] == 0
    assert 0 < free.sum() < len(free)
    assert np.array_equal(opened[0][opened[1]], vc[free])
    assert np.array_equal(opened[2], closed[2][free]) and np.array_equal(opened[3], closed[3][free])


# ------------------------------------------------------------------------------------------------ the kernel stand-in
class MeshStandIn:
    """hip.mesh_faces on CPU tensors, from the restatement."""

    def __init__(self):
        self.calls = []

    def install(self, monkeypatch):
        monkeypatch.setattr(hip, "mesh_faces", self.faces)
        return self

    def faces(self, labels, cells, cap_unknown=True, cells_host=None):
        assert labels.dtype == torch.uint8 and labels.dim() == 2 and labels.shape[1] == B ** 3 and cells.dtype == torch.int32
        self.calls.append({"rows": int(labels.shape[0]), "grid": tuple(cells.shape), "cap": bool(cap_unknown)})
        return tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in mesh_ref(labels.numpy(), cells.numpy(), cap_unknown))


def assert_ply_is(path, m, colours, voxel_size):
    back = mesh.read_mesh_ply(str(path))
    assert back["voxel_size"] == voxel_size
    assert np.array_equal(back["vertices"], m.world_vertices().astype(np.float32))
    assert np.array_equal(back["faces"], m.quads.numpy()) and np.array_equal(back["label"], m.face_label.numpy())
    assert np.array_equal(back["rgb"], np.asarray(colours)[m.face_label.numpy()])


def test_ply_round_trip_quads_triangles_and_empty(monkeypatch, tmp_path):
    MeshStandIn().install(monkeypatch)
    rng = np.random.default_rng(5)
    labels = torch.from_numpy(rng.integers(0, 4, size=(20, 9, 17)).astype(np.uint8))
    m = mesh.mesh_labels(labels, 0.08, (-1.2, 0.4, 2.0))
    assert m.n_faces > 0 and m.vertices.dtype == torch.int32 and m.vertices[:, 0].max() <= 20
    colours = np.arange(24, dtype=np.uint8).reshape(8, 3)
    assert_ply_is(mesh.write_mesh_ply(str(tmp_path / "q.ply"), m, colours), m, colours, 0.08)
    assert np.allclose(m.world_vertices()[0], (np.array([-1.2, 0.4, 2.0]) / 0.08 + m.vertices[0].numpy()) * 0.08, atol=0, rtol=0)
    tri = mesh.read_mesh_ply(mesh.write_mesh_ply(str(tmp_path / "t.ply"), m, colours, triangles=True))
    q = m.quads.numpy()
    assert np.array_equal(tri["faces"], np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3))
    assert np.array_equal(tri["label"], np.repeat(m.face_label.numpy(), 2)) and len(m.triangles()) == 2 * m.n_faces
    empty = mesh.mesh_labels(torch.zeros((4, 4, 4), dtype=torch.uint8), 0.2, (0, 0, 0))
    back = mesh.read_mesh_ply(mesh.write_mesh_ply(str(tmp_path / "e.ply"), empty, colours))
    assert empty.n_faces == 0 and back["faces"].shape == (0, 4) and back["vertices"].shape == (0, 3)
    with pytest.raises(ValueError, match="no colour"):
        mesh.write_mesh_ply(str(tmp_path / "bad.ply"), m, colours[:2])
    with open(tmp_path / "q.ply", "rb") as f:
        data = f.read()
    with open(tmp_path / "short.ply", "wb") as f:
        f.write(data[:-3])
    with pytest.raises(ValueError, match="announces"):
        mesh.read_mesh_ply(str(tmp_path / "short.ply"))
    # int16 labels and logits take the same path; values above 254 are unknown
    wide = labels.to(torch.int16)
    wide[0, 0, 0] = 300
    known = labels.clone()
    known[0, 0, 0] = 255
    assert_mesh_equal(mesh_parts(mesh.mesh_labels(wide, 0.08, (0, 0, 0))), mesh_parts(mesh.mesh_labels(known, 0.08, (0, 0, 0)), True))
    logits = torch.nn.functional.one_hot(labels.long(), 4).permute(3, 0, 1, 2).float()
    assert_mesh_equal(mesh_parts(mesh.mesh_labels(logits, 0.08, (0, 0, 0))), mesh_parts(m, True))


def mesh_parts(m, host=False):
    parts = (m.vertices, m.quads, m.face_label, m.face_dir)
    return tuple(p.numpy() for p in parts) if host else parts


# ------------------------------------------------------------------------------------------------ hook and tools
def _hook_world(monkeypatch, tmp_path):
    KernelStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    root = tmp_path / "sequences"
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    _write_sequence(root / "08", line % (0, 0) + line % (0.2, 0.4) + line % (-0.2, 1.0))
    _write_sequence(root / "03", line % (0, 0) + line % (0.4, 0.2))
    return root


def _closed_face_count(points):
    """Faces of the closed surface of a set of voxels: six per voxel less one per solid neighbour."""
    have = {tuple(p) for p in points.tolist()}
    return sum(tuple(np.add(p, n)) not in have for p in have for n in NORMALS.tolist())


def test_model_hook_writes_meshes_only_when_switched_on(monkeypatch, tmp_path):
    from occdepth_amd.models.OccDepth import OccDepth
    root = _hook_world(monkeypatch, tmp_path)
    k = MeshStandIn().install(monkeypatch)
    steps = _hook_steps()
    off = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "off"), str(root))
    assert off.semantic_map["mesh"] is False
    _epoch(off, "val", steps)
    assert not k.calls and not [n for n in os.listdir(tmp_path / "off") if "mesh" in n]
    on = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "on"), str(root), mesh=True)
    _epoch(on, "val", steps)
    meshes = ["val_%s_%s_mesh.ply" % (s, r) for s in ("03", "08") for r in ("gt", "pred")]
    assert sorted(n for n in os.listdir(tmp_path / "on") if "mesh" in n) == meshes
    assert sorted(os.path.basename(p) for p in on.semantic_map["paths"] if p.endswith("_mesh.ply")) == meshes
    assert len(k.calls) == 4 and all(c["cap"] for c in k.calls)
    for name in meshes:                                                        # against the point PLY of the same map
        points, vs = sm.read_ply(str(tmp_path / "on" / name.replace("_mesh", "")))
        back = mesh.read_mesh_ply(str(tmp_path / "on" / name))
        centres = np.stack([points["x"], points["y"], points["z"]], -1).astype(np.float64) / vs - 0.5
        assert back["voxel_size"] == vs and len(back["faces"]) == _closed_face_count(np.rint(centres).astype(np.int64)) > 0
        assert set(back["label"].tolist()) <= set(points["label"].tolist()) and (edge_use(back["faces"]) % 2 == 0).all()
        low = np.rint(back["vertices"].astype(np.float64).min(0) / vs)
        assert np.array_equal(low, np.rint(centres).min(0))


def test_model_hook_rank_zero_alone_writes_after_the_merge(monkeypatch, tmp_path):
    import torch.distributed as dist
    from occdepth_amd.models.OccDepth import OccDepth
    root = _hook_world(monkeypatch, tmp_path)
    events = []
    k = MeshStandIn()
    monkeypatch.setattr(hip, "mesh_faces", lambda *a, **kw: (events.append("mesh"), k.faces(*a, **kw))[1])
    monkeypatch.setattr(sm, "merge_over_ranks", lambda m, *a, **kw: (events.append("merge"), m)[1])
    rank = {"r": 0}
    for name, fn in (("is_available", lambda: True), ("is_initialized", lambda: True), ("get_world_size", lambda *a: 2),
                     ("get_rank", lambda *a: rank["r"])):
        monkeypatch.setattr(dist, name, fn)
    monkeypatch.setattr(dist, "all_gather_object", lambda out, obj, *a: out.__setitem__(slice(None), [obj, ({}, [])]))
    for r in (0, 1):
        rank["r"] = r
        del events[:]
        stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / ("rank%d" % r)), str(root), mesh=True)
        _epoch(stub, "val", _hook_steps())
        names = os.listdir(tmp_path / ("rank%d" % r))
        if r == 0:
            assert len([n for n in names if n.endswith("_mesh.ply")]) == 4
            assert events == ["merge"] * 4 + ["mesh"] * 4                      # two sequences x (prediction, ground truth)
        else:
            assert names == [] and "mesh" not in events and not stub.semantic_map["paths"]


def test_model_switch_in_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth
    cfg, _ = gc.occdepth_config("kitti_flosp_small")

    def model():
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg)
    for var in ("OCCDEPTH_MAP_DIR", "OCCDEPTH_MAP_POSES", "OCCDEPTH_MAP_MESH", "OCCDEPTH_FUSE", "OCCDEPTH_FUSE_POSES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OCCDEPTH_MAP_MESH", "1")
    assert model().semantic_map is None                                        # the mesh rides on the map's own switch
    monkeypatch.setenv("OCCDEPTH_MAP_DIR", str(tmp_path / "maps"))
    monkeypatch.setenv("OCCDEPTH_MAP_POSES", str(tmp_path / "seq"))
    assert model().semantic_map["mesh"] is True
    monkeypatch.delenv("OCCDEPTH_MAP_MESH")
    assert model().semantic_map["mesh"] is False


@pytest.mark.parametrize("opened", [False, True])
def test_map_sequence_tool_writes_the_meshes_of_its_maps(monkeypatch, tmp_path, opened):
    tool = _tool()
    KernelStandIn().install(monkeypatch)
    k = MeshStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    dims, C = (16, 12, 8), 20
    seq = _write_sequence(tmp_path / "08", "1 0 0 0 0 1 0 0 0 0 1 0\n1 0 0 0 0 1 0 0 0 0 1 0.4\n1 0 0 0.2 0 1 0 0 0 0 1 1.0\n")
    pkl = tmp_path / "pkl"
    os.makedirs(pkl)
    for n, (lab, mask) in enumerate(frames_for(dims, C, 21, 3, masked=True)):
        with open(pkl / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": lab.astype(np.uint16), "target": np.roll(lab, 1, axis=0).astype(np.uint16),
                         "fov_mask_1": mask.reshape(-1)}, f)
    base = ["--poses", seq, "--pred", str(pkl), "--gt", str(pkl), "--out", str(tmp_path / "m" / "08"), "--dims", "16", "12", "8",
            "--origin"] + [str(o) for o in GRIDS[dims]]
    tool.run(tool.parser().parse_args(base), device=torch.device("cpu"))
    assert not k.calls and not [n for n in os.listdir(tmp_path / "m") if "mesh" in n]                 # off is off
    maps, _ = tool.run(tool.parser().parse_args(base + ["--mesh"] + (["--mesh-open"] if opened else [])), device=torch.device("cpu"))
    assert sorted(n for n in os.listdir(tmp_path / "m") if "mesh" in n) == ["08_gt_mesh.ply", "08_pred_mesh.ply"]
    assert [c["cap"] for c in k.calls] == [not opened] * 2
    volume = sm.MapVolume(maps["pred"], maps["gt"], 1, drop_empty=False)
    colours = tool.render.palette("kitti").numpy()
    for role, vol in (("pred", volume), ("gt", volume.target_volume())):
        want = mesh.Mesh(*(torch.from_numpy(a) for a in mesh_ref(vol.labels.numpy(), vol.cells.numpy(), not opened)),
                         vol.origin_voxels, vol.voxel_size)
        assert want.n_faces > 0
        assert_ply_is(tmp_path / "m" / ("08_%s_mesh.ply" % role), want, colours, vol.voxel_size)
    # a brick of observed free space stays free: mesh_map keeps it in the directory
    assert int((volume.cells >= 0).sum()) == volume.n_rows
    only = tool.run(tool.parser().parse_args(base[:4] + base[6:] + ["--mesh"]), device=torch.device("cpu"))
    assert only[1] is None and os.path.exists(tmp_path / "m" / "08_pred_mesh.ply")


def test_render_predictions_tool_writes_one_mesh_per_frame(monkeypatch, tmp_path):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "render_predictions.py")
    spec = importlib.util.spec_from_file_location("render_predictions_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    k = MeshStandIn().install(monkeypatch)
    rng = np.random.default_rng(9)
    labels = rng.integers(0, 5, size=(20, 12, 8)).astype(np.uint8)
    for dataset, frame, origin in (("kitti", {}, (0.0, -0.5 * 0.4 * 12, -2.0)),
                                   ("NYU", {"vox_origin": np.array([0.5, -1.0, 0.25])}, (0.5, -1.0, 0.25))):
        stem = str(tmp_path / dataset)
        out = tool.write_frame_mesh(stem, torch.from_numpy(labels).to(torch.int16), frame, 0.4, dataset)
        assert out == stem + "_mesh.ply"
        rows, cells = mesh.brick_rows(torch.from_numpy(labels))
        assert tuple(cells.shape) == (2, 1, 1) and int((rows.reshape(2, B, B, B)[1, 4:] != 255).sum()) == 0
        want = mesh.Mesh(*(torch.from_numpy(a) for a in mesh_ref(rows.numpy(), cells.numpy())), np.array(origin) / 0.4, 0.4)
        assert_ply_is(out, want, tool.render.palette(dataset).numpy(), 0.4)
    assert len(k.calls) == 2
    assert "--mesh" in open(path).read() and "args.mesh" in open(path).read()


# ------------------------------------------------------------------------------------------------ argument checks
def test_mesh_entry_points_validate_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected
    host = np.full((3, 3, 2), -1, dtype=np.int32)

    def args(**kw):
        a = hip.MeshArgs()
        for f in ("labels", "cells", "row_cell", "counts", "offsets", "face_label", "face_dir", "keys_lo", "keys_hi", "refs", "marks",
                  "ranks", "quads", "vertices"):
            setattr(a, f, ptr)
        a.gx, a.gy, a.gz, a.n_rows, a.cap_unknown, a.n_faces, a.n_vertices = 3, 3, 2, 10, 1, 100, 200
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    grid = (("gx", 0), ("gy", -1), ("gz", 0), ("gx", 65537), ("gz", 65537))
    volume = (("labels", None), ("cells", None), ("row_cell", None), ("n_rows", 0), ("n_rows", -4), ("labels", ptr + 4))
    corners = (("keys_lo", None), ("n_faces", 0), ("n_faces", -1), ("n_faces", 1 << 29), ("n_faces", 1 << 40))
    own = {"occd_mesh_count": grid + volume + (("counts", None),),
           "occd_mesh_emit": grid + volume + corners + (("offsets", None), ("face_label", None), ("face_dir", None), ("refs", None),
                                                        ("keys_lo", ptr + 4), ("refs", ptr + 8)),
           "occd_mesh_heads": grid + corners + (("marks", None),),
           "occd_mesh_weld": grid + corners + (("refs", None), ("ranks", None), ("quads", None), ("vertices", None),
                                               ("n_vertices", 0), ("n_vertices", -2))}
    for name, cases in own.items():
        fn = getattr(hip_lib, name)
        assert fn(None, None) == -1
        for field, value in cases:
            assert fn(ctypes.byref(args(**{field: value})), None) == -1, (name, field, value)
        over = args(gx=2048, gy=2048, gz=64)                                   # 2^28 cells
        assert fn(ctypes.byref(over), None) == -1, name
        wide = args(gx=2048, gy=2048, gz=1, keys_hi=None)                      # a 37-bit key without its high words
        if name != "occd_mesh_count":
            assert fn(ctypes.byref(wide), None) == -1, name
    for fn in (hip_lib.occd_mesh_count, hip_lib.occd_mesh_emit):               # the host copy of the directory
        for bad in (10, 1 << 20):
            host[2, 1, 1] = bad
            assert fn(ctypes.byref(args(cells_host=host.ctypes.data)), None) == -1, bad
        host[2, 1, 1] = -1
    # the key of the largest window the directory allows: the 63-bit limit cannot be reached through the grid limits
    assert max(sum(hip.mesh_key_bits(g)) for g in ((65536, 2048, 1), (512, 512, 512), (65536, 1, 2048))) == 42 < hip.MESH_MAX_KEY_BITS
    assert hip.mesh_key_bits((68, 68, 3)) == (11, 11, 6) and sum(hip.mesh_key_bits((2048, 2048, 1))) == 37
    assert hip.ABI_VERSION == 22 and ctypes.sizeof(hip.MeshArgs) == 15 * 8 + 2 * 8 + 5 * 4 + 4
    for name in own:
        assert name in hip.EXPORTS


def test_wrapper_refuses_what_the_sort_or_the_directory_cannot_take(monkeypatch):
    labels = torch.zeros((2, B ** 3), dtype=torch.uint8)
    cells = torch.tensor([0, 1], dtype=torch.int32).reshape(2, 1, 1)
    emitted = []
    monkeypatch.setattr(hip, "mesh_emit", lambda *a, **kw: emitted.append(a))
    monkeypatch.setattr(hip, "mesh_count", lambda *a, **kw: (torch.tensor([1 << 28, 1 << 28], dtype=torch.int32), None))
    with pytest.raises(ValueError, match="key_range"):                         # 4 F = 2^31
        hip.mesh_faces(labels, cells)
    monkeypatch.setattr(hip, "mesh_count", lambda *a, **kw: (torch.zeros(2, dtype=torch.int32), None))
    out = hip.mesh_faces(labels, cells)                                        # no face: nothing after the count
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 4), (0,), (0,)] and not emitted
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.uint8, torch.uint8]
    for shape in ((65537, 1, 1), (1, 1, 65537)):
        with pytest.raises(ValueError, match="key_range"):
            hip.mesh_faces(labels, torch.zeros(shape, dtype=torch.int32))
    with pytest.raises(ValueError, match="key_range"):
        hip.mesh_key_bits((4096, 4096, 16))                                    # 2^28 cells
