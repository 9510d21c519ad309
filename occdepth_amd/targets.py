"""Training targets of the SemanticKITTI dataloader, built on the GPU (csrc/targets.hip).

The reference builds two supervision targets per sample in numpy inside its dataloader workers, ~3.8 s of CPU per
sample and 142.6 MB shipped per sample at the shipped KITTI geometry (256 x 256 x 32, frustum_size 8):
  * frustum masks and class counts  -- compute_local_frustums, occdepth/data/utils/helpers.py:183-260, called at
    occdepth/data/semantic_kitti/kitti_dataset.py:315-333 (the frustum-proportion loss, `fp_loss`);
  * the CRP relation matrix         -- compute_CP_mega_matrix, helpers.py:6-91, on the 1:8 labels that
    `_downsample_label` (occdepth/data/NYU/preprocess.py:102-143) makes from the 1:1 labels, kitti_dataset.py:294-300
    (the relation loss, `context_prior`).
Both are pure functions of what a batch already carries (`target`, `cam_k`, `T_velo_2_cam`).  The builders here are
bit-exact restatements, GPU only (no CPU path, like hip.py), and never synchronise the host, so they can sit inside a
captured training step.  `OccDepth.step` calls them when a batch comes without the targets (OCCDEPTH_GPU_TARGETS);
`defer_dataset_targets` takes the numpy work out of the reference's dataset.

`kitti_labels` goes one step further back: it makes `target` (and `occluded`) from the dataset's own raw voxel files
(`voxels/<frame>.label`, `.invalid`, `.occluded`), which the reference only reads in a separate preprocessing pass over all
sequences (occdepth/data/semantic_kitti/preprocess.py).  A batch that carries the raw files (`read_raw_kitti_voxels`) needs
no `labels/` tree; tools/preprocess_kitti_gpu.py writes that tree with the same kernels for whoever wants it.
"""
import ctypes
import importlib
import os

import numpy as np
import torch

from . import hip

KITTI_DATASET_MODULE = "occdepth.data.semantic_kitti.kitti_dataset"


def _dev_stack(x, name, dtype=None):
    t = torch.stack(list(x)) if isinstance(x, (list, tuple)) else x
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the target builders have no CPU path)")
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def frustum_targets(cam_E, cam_k, target, *, vox_origin, voxel_size, img_wh, frustum_size, n_classes):
    """compute_local_frustums (helpers.py:183-260, dataset "kitti") for a batch, on the GPU.

    cam_E (B, V, 4, 4) and cam_k (B, V, 3, 3): device tensors (or lists of per-sample (V, ., .) tensors), V = 1 or 2,
    used in float64 (the dataloader's calibration is float64; float32 extrinsics move a few voxels by one pixel).
    target (B, X, Y, Z) labels, 255 = unlabelled.  The projection is the dataloader's vox2pix (pattern point 0,
    helpers.py:94-169; csrc/project.h) at `vox_origin` / `voxel_size` for an image of img_wh = (W, H).
    Returns masks (B, F, X, Y, Z) bool and dists (B, F, n_classes) float32, F = frustum_size ** 2, frustum f = j * s + i
    for x tile i and y tile j (helpers.py:219-220); a voxel is in a frustum when any view puts it there."""
    E = _dev_stack(cam_E, "cam_E", torch.float64)
    K = _dev_stack(cam_k, "cam_k", torch.float64)
    tgt = _dev_stack(target, "target", torch.uint8)
    if E.dim() != 4 or tuple(E.shape[2:]) != (4, 4) or tuple(K.shape) != tuple(E.shape[:2]) + (3, 3):
        raise RuntimeError("frustum_targets: cam_E must be (B, V, 4, 4) and cam_k (B, V, 3, 3)")
    if tgt.dim() != 4 or tgt.shape[0] != E.shape[0]:
        raise RuntimeError("frustum_targets: target must be (B, X, Y, Z) with the batch of cam_E")
    B, V = E.shape[:2]
    X, Y, Z = (int(d) for d in tgt.shape[1:])
    s, C = int(frustum_size), int(n_classes)
    F = s * s
    masks = torch.empty((B, F, X, Y, Z), dtype=torch.uint8, device=tgt.device)
    dists = torch.empty((B, F, C), dtype=torch.float32, device=tgt.device)
    a = hip.FrustumArgs()
    a.cam_E, a.cam_k, a.target, a.masks, a.dists = E.data_ptr(), K.data_ptr(), tgt.data_ptr(), masks.data_ptr(), \
        dists.data_ptr()
    for j, o in enumerate(vox_origin):
        a.vox_origin[j] = float(o)
    a.voxel_size = float(voxel_size)
    a.batch, a.n_views, a.X, a.Y, a.Z = B, V, X, Y, Z
    a.img_w, a.img_h = int(img_wh[0]), int(img_wh[1])
    a.frustum_size, a.n_classes = s, C
    hip._check(hip.load().occd_frustum_targets(ctypes.byref(a), hip._stream()), "occd_frustum_targets")
    return masks.view(torch.bool), dists


def downsample_label(target, ds):
    """_downsample_label (occdepth/data/NYU/preprocess.py:102-143) on the GPU: (B, X, Y, Z) or (X, Y, Z) labels ->
    (B, X/ds, Y/ds, Z/ds) uint8.  Per ds^3 block: more than 95 % of 0 / 255 -> 0 if #0 > #255 else 255, otherwise the most
    frequent label in 1..254 (the smallest on a tie, as np.argmax(np.bincount(...)))."""
    tgt = _dev_stack(target, "target", torch.uint8)
    squeeze = tgt.dim() == 3
    if squeeze:
        tgt = tgt.unsqueeze(0)
    if tgt.dim() != 4:
        raise RuntimeError("downsample_label: target must be (B, X, Y, Z) or (X, Y, Z)")
    B, X, Y, Z = (int(d) for d in tgt.shape)
    ds = int(ds)
    out = torch.empty((B, X // max(ds, 1), Y // max(ds, 1), Z // max(ds, 1)), dtype=torch.uint8, device=tgt.device)
    hip._check(hip.load().occd_downsample_label(tgt.data_ptr(), out.data_ptr(), B, X, Y, Z, ds, hip._stream()),
               "occd_downsample_label")
    return out[0] if squeeze else out


def cp_mega_matrix(coarse, binary=False):
    """compute_CP_mega_matrix (helpers.py:6-91) on the GPU: (B, X, Y, Z) or (X, Y, Z) labels -> (B, R, N, M) uint8 in
    the reference's layout (R = 4, or 2 with `binary`; N = X*Y*Z rows; M = (X/2)(Y/2)(Z/2) mega voxels)."""
    lab = _dev_stack(coarse, "coarse", torch.uint8)
    squeeze = lab.dim() == 3
    if squeeze:
        lab = lab.unsqueeze(0)
    if lab.dim() != 4:
        raise RuntimeError("cp_mega_matrix: labels must be (B, X, Y, Z) or (X, Y, Z)")
    B, X, Y, Z = (int(d) for d in lab.shape)
    R = 2 if binary else 4
    out = torch.empty((B, R, X * Y * Z, (X // 2) * (Y // 2) * (Z // 2)), dtype=torch.uint8, device=lab.device)
    hip._check(hip.load().occd_cp_mega_matrix(lab.data_ptr(), out.data_ptr(), B, X, Y, Z, int(bool(binary)),
                                              hip._stream()), "occd_cp_mega_matrix")
    return out[0] if squeeze else out


# ------------------------------------------------------------------------------------------------ raw voxel labels
# `learning_map` of the SemanticKITTI label definition (semantic-kitti.yaml): raw label -> training class.
KITTI_LEARNING_MAP = ((0, 0), (1, 0), (10, 1), (11, 2), (13, 5), (15, 3), (16, 5), (18, 4), (20, 5), (30, 6), (31, 7),
                      (32, 8), (40, 9), (44, 10), (48, 11), (49, 12), (50, 13), (51, 14), (52, 0), (60, 9), (70, 15),
                      (71, 16), (72, 17), (80, 18), (81, 19), (99, 0), (252, 1), (253, 7), (254, 6), (255, 8), (256, 5),
                      (257, 5), (258, 4), (259, 5))
KITTI_LUT_LEN = 359               # the largest raw label + 100 (io_data.py:187)


def kitti_remap_lut():
    """The table of io_data.get_remap_lut (io_data.py:175-195) as uint8[359]: raw label -> training class; every raw label
    that maps to class 0, and every label the map does not name, becomes 255 ("invalid"); only raw 0 ("empty") stays 0."""
    lut = np.full(KITTI_LUT_LEN, 255, dtype=np.uint8)
    for raw, cls in KITTI_LEARNING_MAP:
        if cls != 0:
            lut[raw] = cls
    lut[0] = 0
    return lut


_LUT_CACHE = {}


def _device_lut(device):
    key = str(device)
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = torch.from_numpy(kitti_remap_lut()).to(device)
    return _LUT_CACHE[key]


def _raw_rows(x, name, dtypes, cols=None):
    """(B, n) contiguous device tensor of one of `dtypes` from a tensor or a list of per-sample tensors; never converted
    (the kernel reads the files' own bits)."""
    t = x
    if isinstance(x, (list, tuple)):
        rows = [v.reshape(-1) for v in x]
        if rows and all(v.dtype == torch.uint16 for v in rows):      # stacked as int16: the same bits, and every backend has it
            t = torch.stack([v.view(torch.int16) for v in rows]).view(torch.uint16)
        else:
            t = torch.stack(rows)
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the label decode has no CPU path)")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or (cols is not None and tuple(t.shape) != cols):
        raise RuntimeError(f"{name} must be (B, n) with one flat row per sample"
                           + (f", here {cols}" if cols is not None else "") + f"; got {tuple(t.shape)}")
    return t.contiguous()


def kitti_labels_counted(raw, invalid_bits, occluded_bits=None, *, scene_size, lut=None):
    """`kitti_labels` with its device counter: -> (target, occluded or None, count); count is an int32[1] device tensor, the
    number of raw values outside the table, set by every launch and not read here."""
    X, Y, Z = (int(d) for d in scene_size)
    N = X * Y * Z
    if N <= 0 or N % 8:
        raise RuntimeError(f"kitti_labels: the voxel count {N} of scene_size {tuple(scene_size)} must be a positive "
                           "multiple of 8 (the masks are packed 8 voxels to the byte)")
    r = _raw_rows(raw, "raw", (torch.uint16, torch.int16))
    if r.shape[1] != N:
        raise RuntimeError(f"kitti_labels: raw must be (B, {N}) for scene_size {(X, Y, Z)}, got {tuple(r.shape)}")
    B = int(r.shape[0])
    inv = _raw_rows(invalid_bits, "invalid_bits", (torch.uint8,), (B, N // 8))
    occ = None if occluded_bits is None else _raw_rows(occluded_bits, "occluded_bits", (torch.uint8,), (B, N // 8))
    if lut is None:
        table = _device_lut(r.device)
    else:
        table = torch.as_tensor(lut)
        if table.dtype != torch.uint8 or table.dim() != 1 or table.numel() < 1:
            raise RuntimeError("kitti_labels: lut must be a non-empty 1-D uint8 table")
        table = table.to(r.device).contiguous()
    target = torch.empty((B, X, Y, Z), dtype=torch.uint8, device=r.device)
    occluded = None if occ is None else torch.empty((B, X, Y, Z), dtype=torch.uint8, device=r.device)
    count = torch.empty(1, dtype=torch.int32, device=r.device)
    hip._check(hip.load().occd_kitti_labels(r.data_ptr(), inv.data_ptr(), None if occ is None else occ.data_ptr(),
                                            table.data_ptr(), int(table.numel()), target.data_ptr(),
                                            None if occluded is None else occluded.data_ptr(), count.data_ptr(), B, N,
                                            hip._stream()), "occd_kitti_labels")
    return target, occluded, count


def kitti_labels(raw, invalid_bits, occluded_bits=None, *, scene_size, lut=None, check=False):
    """Raw SemanticKITTI voxel files -> training labels on the GPU (occd_kitti_labels), one launch for the batch.

    raw (B, N) uint16 -- or int16 holding the same bits -- the `.label` files, N = X * Y * Z of scene_size, flat in
    (X, Y, Z) order; invalid_bits (B, N / 8) uint8, the `.invalid` files as stored (MSB first, io_data.unpack);
    occluded_bits optional, the `.occluded` files.  Lists of per-sample tensors are stacked.  Returns
    target (B, X, Y, Z) uint8 = lut[raw], 255 where the invalid bit is set -- the values of the reference's
    `<frame>_1_1.npy` (preprocess.py:76-84) -- and, with occluded_bits, (target, occluded (B, X, Y, Z) uint8 of 0 / 1).
    `lut` defaults to kitti_remap_lut().  A raw value outside the table gives 255 and is counted on the device; with
    `check` the count is read back (a host synchronisation: tools only, never the training step) and a non-zero count
    raises IndexError, as the reference's table lookup would."""
    target, occluded, count = kitti_labels_counted(raw, invalid_bits, occluded_bits, scene_size=scene_size, lut=lut)
    if check:
        bad = int(count.item())
        if bad:
            raise IndexError(f"kitti_labels: {bad} raw label(s) lie outside the remap table")
    return target if occluded is None else (target, occluded)


def read_raw_kitti_voxels(voxel_dir, frame_id, occluded=False):
    """The raw voxel files of one frame, undecoded, for a dataset's __getitem__: (`<frame>.label` as uint16[N],
    `<frame>.invalid` as uint8[N / 8] [, `<frame>.occluded` as uint8[N / 8]]) numpy arrays -- the batch entries
    `voxel_label_raw`, `voxel_invalid_bits` [, `voxel_occluded_bits`] that OccDepth.step decodes on the GPU."""
    base = os.path.join(voxel_dir, frame_id)
    out = (np.fromfile(base + ".label", dtype=np.uint16), np.fromfile(base + ".invalid", dtype=np.uint8))
    if occluded:
        out += (np.fromfile(base + ".occluded", dtype=np.uint8),)
    return out


# ------------------------------------------------------------------------------------------------ dataset hook
def _no_frustums(*args, **kwargs):
    """Stands in for compute_local_frustums: no masks, so the reference collate skips them (collate.py:29-34)."""
    return None, None


def _no_cp_matrix(*args, **kwargs):
    """Stands in for compute_CP_mega_matrix: a zero-size uint8 array (collate.py:59-60 still calls torch.from_numpy)."""
    return np.zeros((0,), dtype=np.uint8)


class DatasetTargetsHook:
    """Undo handle of `defer_dataset_targets`: `undo()` restores the names it rebound (idempotent)."""

    def __init__(self, module, saved):
        self.module, self.saved = module, saved

    @property
    def active(self):
        return self.module is not None and bool(self.saved)

    def undo(self):
        if self.module is not None:
            for name, fn in self.saved.items():
                setattr(self.module, name, fn)
        self.saved = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.undo()


def defer_dataset_targets(module=None):
    """Rebind `compute_local_frustums` and `compute_CP_mega_matrix` inside the reference's SemanticKITTI dataset module
    (occdepth.data.semantic_kitti.kitti_dataset, when importable; or `module`) to stubs, so its workers stop building the
    frustum and relation targets; `OccDepth.step` then builds them on the GPU (OCCDEPTH_GPU_TARGETS).  Returns a
    DatasetTargetsHook (inactive when the module cannot be imported).

    Only the module's global names change, in this process: dataloader workers started by fork afterwards inherit them;
    workers started before the call, or by spawn / forkserver, do not.  Install the hook before the first epoch's
    workers start (OCCDEPTH_GPU_TARGETS=1 installs it when the model is constructed)."""
    if module is None:
        try:
            module = importlib.import_module(KITTI_DATASET_MODULE)
        except Exception:
            return DatasetTargetsHook(None, {})
    return _rebind(module, (("compute_local_frustums", _no_frustums), ("compute_CP_mega_matrix", _no_cp_matrix)))


def _rebind(module, stubs):
    saved = {}
    for name, stub in stubs:
        if hasattr(module, name) and getattr(module, name) is not stub:
            saved[name] = getattr(module, name)
            setattr(module, name, stub)
    return DatasetTargetsHook(module, saved)


def _no_vox2pix(*args, **kwargs):
    """Stands in for vox2pix (helpers.py:94-169): zero-size tables of the real ranks and dtypes -- projected_pix (0, 1, 2)
    int64, fov_mask (0, 1) bool, pix_z (0,) float64 -- which survive the dataset's flip line (kitti_dataset.py:388) and
    the collate's torch.from_numpy; OccDepth treats zero-element tables as absent and projects on the GPU."""
    return np.zeros((0, 1, 2), dtype=np.int64), np.zeros((0, 1), dtype=bool), np.zeros((0,), dtype=np.float64)


def defer_dataset_projection(module=None):
    """Rebind `vox2pix` and `compute_local_frustums` inside the reference's SemanticKITTI dataset module (when importable;
    or `module`) to stubs, so its workers stop building and shipping the voxel -> pixel tables (about 80 MB per sample at
    config 2); `OccDepth` then builds them on the GPU (occd_vox2pix, flip included).  compute_local_frustums reads those
    tables, so it is stubbed as in `defer_dataset_targets` and the frustum targets come from the GPU builders
    (OCCDEPTH_GPU_TARGETS must not be 0).  Returns a DatasetTargetsHook (undo, context manager; inactive when the module
    cannot be imported).  The same process / fork caveats as `defer_dataset_targets` apply; OCCDEPTH_GPU_PROJECTION=1
    installs it when the model is constructed."""
    if module is None:
        try:
            module = importlib.import_module(KITTI_DATASET_MODULE)
        except Exception:
            return DatasetTargetsHook(None, {})
    return _rebind(module, (("vox2pix", _no_vox2pix), ("compute_local_frustums", _no_frustums)))


def _no_depth(*args, **kwargs):
    """Stands in for load_depth (kitti_dataset.py:40-44): a zero-size float32 map, which survives the dataset's crop and
    np.fliplr (kitti_dataset.py:338-348) and the collate's torch.stack; OccDepth treats a zero-element `gt_depth` as
    absent and matches the batch's image pair on the GPU."""
    return np.zeros((0, 0), dtype=np.float32)


def defer_dataset_stereo_depth(module=None):
    """Rebind `load_depth` inside the reference's SemanticKITTI dataset module (when importable; or `module`) to a stub,
    so its workers stop reading the per-frame stereo depth PNGs -- files of a side dataset the user may not have;
    `OccDepth.step` then builds the depth target from the batch's image pair (stereo.stereo_depth, OCCDEPTH_GPU_STEREO).
    Returns a DatasetTargetsHook (undo, context manager; inactive when the module cannot be imported).  The same process
    / fork caveats as `defer_dataset_targets` apply; OCCDEPTH_GPU_STEREO=1 installs it when the model is constructed."""
    if module is None:
        try:
            module = importlib.import_module(KITTI_DATASET_MODULE)
        except Exception:
            return DatasetTargetsHook(None, {})
    return _rebind(module, (("load_depth", _no_depth),))
