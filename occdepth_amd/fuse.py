"""Temporal fusion of predictions over a sequence: the class probabilities of earlier key frames are warped into the
current frame's voxel grid with the ego-motion (nearest voxel) and combined per voxel on the GPU (csrc/fuse.hip:
hip.fuse_store keeps a frame's softmax in a ring slot, hip.fuse_frames gathers and combines in one launch).

    poses = read_kitti_poses(".../dataset/sequences/08")             # {frame: 4 x 4}, velodyne frame
    fuser = SequenceFuser((256, 256, 32), 20, (0.0, -25.6, -2.0), 0.2, window=4)
    out = fuser.push(ssc_logit[i], poses[frame], key=("08", frame), fov_mask=fov_mask_1[i])
    out["y_pred"], out["n_obs"]                                      # (X, Y, Z) uint8, on the GPU

The host side is numpy in float64; the 12 coefficients per source travel by value with the launch.  The effect on mIoU
is not measured (no checkpoint and no dataset where this was built): the module delivers the mechanism and its cost.
"""
import os

import numpy as np
import torch

from . import hip


# ----------------------------------------------------------------------------------------------------- poses
def _rigid_inverse(T):
    """4 x 4 rigid transform -> its inverse as R^T, -R^T t (no matrix inversion; render.camera_view does the same)."""
    T = np.asarray(T, dtype=np.float64)
    out = np.eye(4, dtype=np.float64)
    Rt = T[:3, :3].T
    out[:3, :3] = Rt
    out[:3, 3] = -Rt @ T[:3, 3]
    return out


def _row12(words, path, what):
    try:
        vals = [float(w) for w in words]
    except ValueError:
        vals = []
    if len(vals) != 12 or len(words) != 12:
        raise ValueError("%s: %s does not hold 12 numbers" % (path, what))
    T = np.eye(4, dtype=np.float64)
    T[:3, :4] = np.asarray(vals, dtype=np.float64).reshape(3, 4)
    return T


def read_kitti_poses(sequence_dir):
    """SemanticKITTI / KITTI odometry `poses.txt` (one line of 12 numbers per frame: the camera-0 pose) and the `Tr:`
    row of `calib.txt` (velodyne -> camera 0) of one sequence directory -> {frame index: 4 x 4 float64} in the VELODYNE
    frame, Tr^-1 P_t Tr: the frame the voxel grid is laid out in.  A missing file, a short line or a missing `Tr:` raises
    an error that names the path."""
    calib_path = os.path.join(sequence_dir, "calib.txt")
    poses_path = os.path.join(sequence_dir, "poses.txt")
    for path in (calib_path, poses_path):
        if not os.path.isfile(path):
            raise FileNotFoundError("%s is missing (temporal fusion reads the ego-motion from it)" % path)
    Tr = None
    with open(calib_path) as f:
        for line in f:
            key, _, rest = line.partition(":")
            if key.strip() == "Tr":
                Tr = _row12(rest.split(), calib_path, "the Tr: row")
    if Tr is None:
        raise ValueError("%s has no Tr: row (velodyne -> camera 0)" % calib_path)
    Tr_inv = _rigid_inverse(Tr)
    poses = {}
    with open(poses_path) as f:
        for n, line in enumerate(l for l in f if l.strip()):
            poses[n] = Tr_inv @ _row12(line.split(), poses_path, "line %d" % (n + 1)) @ Tr
    if not poses:
        raise ValueError("%s holds no pose" % poses_path)
    return poses


def grid_affine(pose_src, pose_dst, vox_origin, voxel_size):
    """The 12 float32 coefficients (A row-major, then b) that take a voxel-centre coordinate of the DESTINATION frame's grid
    (grid units: voxel (i, j, l) has its centre at (i + 1/2, j + 1/2, l + 1/2)) into the SOURCE frame's grid.  Poses are
    4 x 4 sensor -> world; both grids have `vox_origin` (metres, sensor frame) and `voxel_size`.  Composed in float64:
    T = pose_src^-1 pose_dst, A = R(T), b = (R origin + t - origin) / voxel_size."""
    T = _rigid_inverse(pose_src) @ np.asarray(pose_dst, dtype=np.float64)
    R, t = T[:3, :3], T[:3, 3]
    org = np.asarray(vox_origin, dtype=np.float64).reshape(3)
    b = (R @ org + t - org) / float(voxel_size)
    return np.concatenate([R.reshape(9), b]).astype(np.float32)


IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)     # the current frame: exact, whatever its pose


# ----------------------------------------------------------------------------------------------------- the ring
class SequenceFuser:
    """Fuse every pushed frame with up to `window - 1` earlier frames of the same sequence.

    push() stores the frame's softmax in a ring slot (the pass that takes the copy: under a replayed forward graph the
    logits buffer is overwritten by the next forward) and fuses: the current frame contributes everywhere with weight 1,
    the most recent earlier frame with weight decay, the next with decay^2, ..., each only where its own `fov_mask` (kept
    with the slot as uint8) is set and where the warped voxel centre falls inside its grid.

    The ring resets when the sequence changes or the frame index does not increase; an earlier frame more than `max_gap`
    frames back is dropped (with it every older one: when that is the most recent, the ring is empty again).

    Memory: `window` slots of X Y Z pitch float32, allocated on the first push and never regrown -- at 256 x 256 x 32 x 20
    classes 168 MB per slot at pitch 20 (671 MB for window = 4), plus X Y Z bytes per slot for the masks.  The row pitch is
    n_classes rounded up to 4 floats: rows padded to 128 bytes take 60 % more memory and measured slower in the store pass
    and at window 8, and within the spread between runs at windows 2 and 4 (profiles/fuse_ab.txt)."""

    def __init__(self, dims, n_classes, vox_origin, voxel_size, window=4, decay=1.0, max_gap=None, return_prob=False):
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1:
            raise ValueError("dims must be (X, Y, Z), got %r" % (dims,))
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= 32:
            raise ValueError("1..32 classes, got %r" % (n_classes,))
        self.window = int(window)
        if not 1 <= self.window <= hip.FUSE_MAX_SOURCES:
            raise ValueError("window must be 1..%d, got %r" % (hip.FUSE_MAX_SOURCES, window))
        self.decay = float(decay)
        if not 0.0 < self.decay <= 1.0:
            raise ValueError("decay must be in (0, 1], got %r" % (decay,))
        self.max_gap = None if max_gap is None else int(max_gap)
        if self.max_gap is not None and self.max_gap < 1:
            raise ValueError("max_gap must be >= 1, got %r" % (max_gap,))
        self.pitch = hip.round_up(self.n_classes, 4)
        self.vox_origin = tuple(float(v) for v in np.asarray(vox_origin, dtype=np.float64).reshape(3))
        self.voxel_size = float(voxel_size)
        self.return_prob = bool(return_prob)
        self.rows = self.masks = None        # (window, S, pitch) float32 / (window, S) uint8, with the first push
        self.entries = []                    # newest first: {"slot", "frame", "pose", "mask"}
        self.sequence = None

    def reset(self):
        self.entries = []
        self.sequence = None

    def _admit(self, sequence, frame):
        """Apply the reset rules for a frame about to be pushed and return the ring slot it takes."""
        if self.entries and (sequence != self.sequence or frame <= self.entries[0]["frame"]):
            self.entries = []
        self.sequence = sequence
        if self.max_gap is not None:
            self.entries = [e for e in self.entries if frame - e["frame"] <= self.max_gap]
        self.entries = self.entries[:self.window - 1]
        used = {e["slot"] for e in self.entries}
        return next(s for s in range(self.window) if s not in used)

    def push(self, ssc_logit_i, pose, key, fov_mask=None):
        """ssc_logit_i: (C, X, Y, Z) float32 logits of one frame on the GPU (planes or the channels-last view the eval
        path returns); pose: 4 x 4 sensor -> world; key = (sequence, frame index); fov_mask: the frame's own (X Y Z) FOV
        table (bool / uint8, any shape).  -> {"y_pred": (X, Y, Z) uint8 labels, "n_obs": (X, Y, Z) uint8 number of frames
        that contributed[, "ssc_prob": (X, Y, Z, C) float32 fused probabilities]}."""
        C, dims = self.n_classes, self.dims
        if tuple(ssc_logit_i.shape) != (C,) + dims:
            raise ValueError("push takes (C, X, Y, Z) = %r logits, got %r" % ((C,) + dims, tuple(ssc_logit_i.shape)))
        pose = np.asarray(pose, dtype=np.float64)
        if pose.shape != (4, 4):
            raise ValueError("pose must be 4 x 4, got %r" % (pose.shape,))
        sequence, frame = key[0], int(key[1])
        S = dims[0] * dims[1] * dims[2]
        dev = ssc_logit_i.device
        if self.rows is None:
            self.rows = torch.empty((self.window, S, self.pitch), dtype=torch.float32, device=dev)
            self.masks = torch.empty((self.window, S), dtype=torch.uint8, device=dev)
        slot = self._admit(sequence, frame)
        hip.fuse_store(ssc_logit_i.detach(), self.rows[slot])
        if fov_mask is not None:
            m = torch.as_tensor(fov_mask)
            if m.numel() != S:
                raise ValueError("fov_mask must hold X Y Z = %d entries, got %r" % (S, tuple(m.shape)))
            self.masks[slot].copy_(m.reshape(S).to(dev) != 0)
        earlier = self.entries
        self.entries = [{"slot": slot, "frame": frame, "pose": pose, "mask": fov_mask is not None}] + earlier
        rows = [self.rows[slot]] + [self.rows[e["slot"]] for e in earlier]
        masks = [None] + [self.masks[e["slot"]] if e["mask"] else None for e in earlier]
        weights = [self.decay ** n for n in range(len(rows))]
        affines = [IDENTITY] + \
            [grid_affine(e["pose"], pose, self.vox_origin, self.voxel_size) for e in earlier]
        labels, n_obs, prob = hip.fuse_frames(rows, affines, weights, dims, C, masks=masks, return_prob=self.return_prob)
        out = {"y_pred": labels, "n_obs": n_obs}
        if self.return_prob:
            out["ssc_prob"] = prob[:, :C].reshape(dims + (C,))
        return out
