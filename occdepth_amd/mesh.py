"""Surface meshes of predictions and of the sequence map (K39, csrc/mesh.hip; welded on the radix sort K38).

A `semantic_map.MapVolume` -- or one frame's dense label volume, tiled into the same brick rows -- becomes an indexed quad
mesh: one quad per exposed voxel face, every lattice corner once.  The rules (solid / free / unknown, the face codes, the
order of faces, corners and vertices) are the contract of occd_mesh_count ... occd_mesh_weld in include/occdepth_amd.h;
`hip.mesh_faces` runs the stages.  Everything is integer: the same input gives the same bytes.

    mesh_volume(volume, cap_unknown=True)                      -> Mesh
    mesh_map(pred, gt=None, min_obs=1, key_range=None, ...)    -> Mesh, or (Mesh, Mesh) with a ground-truth map
    mesh_labels(labels, voxel_size, vox_origin, ...)           -> Mesh of one frame
    write_mesh_ply(path, mesh, colours, triangles=False) / read_mesh_ply(path)

cap_unknown=True closes the surface of the solid set (faces towards unobserved space included); False keeps only the faces
where observed free space meets matter.  This module is imported only where a mesh is asked for.
"""
import numpy as np
import torch

from . import hip
from . import semantic_map as sm

BRICK = sm.BRICK
FACE_NORMALS = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], dtype=np.int64)   # by face code


class Mesh:
    """vertices (V, 3) int32 lattice corners of the window, ascending in (x, y, z); quads (F, 4) int32 vertex indices,
    counter-clockwise seen from outside, from the lexicographically smallest corner; face_label (F,) uint8; face_dir (F,)
    uint8 face code (0 .. 5 = -x +x -y +y -z +z); origin_voxels (3,) the window's corner in world voxels; voxel_size in
    metres.  Tensors live on the device of the volume they were made from."""

    __slots__ = ("vertices", "quads", "face_label", "face_dir", "origin_voxels", "voxel_size")

    def __init__(self, vertices, quads, face_label, face_dir, origin_voxels, voxel_size):
        self.vertices, self.quads, self.face_label, self.face_dir = vertices, quads, face_label, face_dir
        self.origin_voxels = np.asarray(origin_voxels).reshape(3)
        self.voxel_size = float(voxel_size)

    @property
    def n_faces(self):
        return int(self.quads.shape[0])

    @property
    def n_vertices(self):
        return int(self.vertices.shape[0])

    def world_vertices(self):
        """(V, 3) float64 on the host: (origin_voxels + corner) * voxel_size, world metres."""
        corner = self.vertices.detach().cpu().numpy().astype(np.float64)
        return (self.origin_voxels.astype(np.float64) + corner) * self.voxel_size

    def triangles(self):
        """(2 F, 3): every quad (0, 1, 2, 3) as (0, 1, 2), (0, 2, 3), faces in order."""
        q = self.quads
        return torch.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 3)


def mesh_volume(volume, cap_unknown=True):
    """The mesh of a semantic_map.MapVolume's labels (its target is not read: mesh `volume.target_volume()` for that)."""
    parts = hip.mesh_faces(volume.labels.reshape(-1, BRICK ** 3), volume.cells, cap_unknown=cap_unknown)
    return Mesh(*parts, volume.origin_voxels, volume.voxel_size)


def mesh_map(pred, gt=None, min_obs=1, key_range=None, cap_unknown=True):
    """The mesh of a SemanticMap (voxels with at least min_obs votes, inside the brick-key box key_range when given).  The
    volume is built with drop_empty=False: a brick of observed free space stays free, so with cap_unknown=False the faces
    towards it are kept.  With `gt` -> (prediction mesh, ground-truth mesh), the second from target_volume()."""
    volume = sm.MapVolume(pred, gt, min_obs, key_range, drop_empty=False)
    mesh = mesh_volume(volume, cap_unknown)
    if gt is None:
        return mesh
    return mesh, mesh_volume(volume.target_volume(), cap_unknown)


def brick_rows(labels):
    """A dense (X, Y, Z) uint8 volume -> ((n, 4096) brick rows, (gx, gy, gz) int32 directory), padded with 255 to whole
    bricks, by torch operators on the volume's device."""
    X, Y, Z = (int(d) for d in labels.shape)
    grid = tuple(-(-d // BRICK) for d in (X, Y, Z))
    padded = torch.full(tuple(BRICK * g for g in grid), 255, dtype=torch.uint8, device=labels.device)
    padded[:X, :Y, :Z] = labels
    rows = padded.reshape(grid[0], BRICK, grid[1], BRICK, grid[2], BRICK).permute(0, 2, 4, 1, 3, 5).reshape(-1, BRICK ** 3)
    cells = torch.arange(rows.shape[0], dtype=torch.int32, device=labels.device).reshape(grid)
    return rows.contiguous(), cells


def mesh_labels(labels, voxel_size, vox_origin, cap_unknown=True):
    """The mesh of one frame: labels (X, Y, Z) uint8 / int16 (values above 254 are unknown), or logits (C, X, Y, Z) whose
    arg-max is taken; vox_origin: the grid's corner in metres.  Any size: the volume is padded to whole bricks."""
    if not torch.is_tensor(labels):
        labels = torch.as_tensor(np.asarray(labels))
    if labels.dim() == 4 and labels.is_floating_point():
        labels = labels.argmax(0)
    if labels.dim() != 3 or labels.is_floating_point() or min(labels.shape) < 1:
        raise ValueError("labels must be an (X, Y, Z) integer volume or (C, X, Y, Z) logits, got %s %s" % (tuple(labels.shape), labels.dtype))
    if labels.dtype != torch.uint8:
        wide = labels.to(torch.int32) & (0xFFFF if labels.dtype == torch.int16 else 0x7FFFFFFF)
        labels = wide.clamp(max=255).to(torch.uint8)
    rows, cells = brick_rows(labels)
    parts = hip.mesh_faces(rows, cells, cap_unknown=cap_unknown)
    origin = np.asarray(vox_origin, dtype=np.float64).reshape(3) / float(voxel_size)
    return Mesh(*parts, origin, voxel_size)


# ----------------------------------------------------------------------------------------------------- PLY
def _face_dtype(k):
    return np.dtype([("n", "u1"), ("v", "<i4", (k,)), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("label", "u1")])


_VERTEX_PROPS = ("float x", "float y", "float z")
_FACE_PROPS = ("list uchar int vertex_indices", "uchar red", "uchar green", "uchar blue", "uchar label")


def write_mesh_ply(path, mesh, colours, triangles=False):
    """A binary little-endian PLY: vertices x y z float32 (world metres), faces `list uchar int vertex_indices` (4 per
    face, or 3 with triangles: two per quad) with uchar red green blue (colours[label]; render.palette) and label.  -> path."""
    verts = mesh.world_vertices().astype("<f4")
    faces = sm._host(mesh.triangles() if triangles else mesh.quads).astype("<i4")
    labels = sm._host(mesh.face_label).reshape(-1).astype(np.uint8)
    if triangles:
        labels = np.repeat(labels, 2)
    colours = sm._host(colours).reshape(-1, 3).astype(np.uint8)
    if len(labels) and int(labels.max()) >= len(colours):
        raise ValueError("label %d has no colour (%d rows)" % (int(labels.max()), len(colours)))
    k = 3 if triangles else 4
    rows = np.empty(len(faces), dtype=_face_dtype(k))
    rows["n"], rows["v"], rows["label"] = k, faces.reshape(-1, k), labels
    rgb = colours[labels]
    rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = ["ply", "format binary_little_endian 1.0", "comment occdepth_amd semantic map voxel_size %r" % mesh.voxel_size,
              "element vertex %d" % len(verts)] + ["property " + p for p in _VERTEX_PROPS] + \
             ["element face %d" % len(rows)] + ["property " + p for p in _FACE_PROPS] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(verts).tobytes())
        f.write(rows.tobytes())
    return path


def read_mesh_ply(path):
    """A file write_mesh_ply wrote -> {"vertices" (V, 3) float32, "faces" (F, 3 or 4) int32, "rgb" (F, 3) uint8, "label"
    (F,) uint8, "voxel_size" (None without the comment line)}."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    lines = data[:end].decode("ascii").splitlines()
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: only binary_little_endian 1.0 is read, got %r" % (path, lines[1]))
    counts, props, voxel_size, element = {}, {"vertex": [], "face": []}, None, None
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            element = w[1]
            counts[element] = int(w[2])
            props.setdefault(element, [])
        elif w[0] == "property":
            props[element].append(" ".join(w[1:]))
        elif w[0] == "comment" and "voxel_size" in w:
            voxel_size = float(w[w.index("voxel_size") + 1])
    if tuple(props["vertex"]) != _VERTEX_PROPS or tuple(props["face"]) != _FACE_PROPS or set(counts) != {"vertex", "face"}:
        raise ValueError("%s does not have the layout write_mesh_ply writes" % path)
    body = data[end + len(b"end_header\n"):]
    nv, nf = counts["vertex"], counts["face"]
    rest = len(body) - 12 * nv
    k = int(body[12 * nv]) if nf and rest > 0 else 4
    if k not in (3, 4) or rest != nf * _face_dtype(k).itemsize:
        raise ValueError("%s: %d bytes of vertices and faces, its header announces %d vertices and %d faces" % (path, len(body), nv, nf))
    verts = np.frombuffer(body, dtype="<f4", count=3 * nv).reshape(nv, 3)
    rows = np.frombuffer(body, dtype=_face_dtype(k), count=nf, offset=12 * nv)
    if nf and not (rows["n"] == k).all():
        raise ValueError("%s mixes faces of different sizes" % path)
    return {"vertices": verts, "faces": rows["v"].reshape(nf, k), "rgb": np.stack([rows["red"], rows["green"], rows["blue"]], -1),
            "label": rows["label"], "voxel_size": voxel_size}
