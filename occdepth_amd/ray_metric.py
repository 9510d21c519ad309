"""RayIoU: score a predicted label volume along sensor rays (K35, csrc/ray_metric.hip).

Voxel IoU rewards thick surfaces and counts a one-voxel depth slip on a thin object as a complete miss.  The ray-based
metric of "Fully Sparse 3D Occupancy Prediction" (Liu et al., 2024; also the CVPR-2024 occupancy challenge) casts the rays
a lidar would cast through the prediction and through the ground truth and compares, per ray, the class and the depth of
the first surface: a ray is a true positive of class c at threshold tau when both volumes hit class c and the two depths
differ by less than tau; per class IoU = TP / (GT + PRED - TP), averaged over the classes and over tau in {1, 2, 4} m.

    dirs = lidar_directions()                                        # (57600, 3) float32, a 64-beam fan over the half-space
    m = RayMetrics(20, 0.2, dirs)
    m.add_batch(pred_labels, target, sensor_origin((0, -25.6, -2), 0.2))    # one launch, counters stay on the GPU
    m.get_stats()["RayIoU"]

Target voxels labelled 255 are unknown: by default a ray that meets one before its target hit is dropped (counted in
`unknown`, scored nowhere); unknown="pass" sees through them, as the prediction's 255 always is.  The direction fan is a
stand-in for a spinning 64-beam sensor, not a calibration table, and no RayIoU of a trained model was computed where this
was built (no checkpoint and no dataset): the module delivers the metric, pinned against its numpy restatement, and its
cost.
"""
import numpy as np
import torch

from . import hip

SCALARS = ("rays", "valid", "unknown", "pred_miss")         # the counters in front of the per-class ones
UNKNOWN_MODES = {"drop": hip.RAY_UNKNOWN_DROP, "pass": hip.RAY_UNKNOWN_PASS}


# ----------------------------------------------------------------------------------------------------- rays and origins
def lidar_directions(beams=64, pitch_deg=(-24.8, 2.0), azimuth_deg=(-90.0, 90.0), azimuth_step_deg=0.2, tile=8):
    """(N, 3) float32 unit vectors of a spinning-lidar-like fan: `beams` pitch angles evenly spaced over pitch_deg (both
    ends included) x the azimuths azimuth_deg[0] + (j + 1/2) azimuth_step_deg inside azimuth_deg; x forward, y left, z up
    (the grid's axes); computed in float64, normalised, then cast.  The defaults resemble an HDL-64E over the half-space
    in front of the sensor, which is what the grid covers (N = 64 x 900); they are a stand-in pattern, not that sensor's
    calibration table.  Order: tile x tile (beam x azimuth) blocks, block after block along the azimuth, then along the
    beams, beam-major inside a block -- so 64 consecutive rays (one wave of K35) are neighbours; tile=None gives plain
    beam-major order (ray = beam * n_azimuth + azimuth).  The two orders are permutations of one another."""
    beams = int(beams)
    n_az = int(round((float(azimuth_deg[1]) - float(azimuth_deg[0])) / float(azimuth_step_deg)))
    if beams < 1 or n_az < 1:
        raise ValueError("lidar_directions needs at least one beam and one azimuth, got %d x %d" % (beams, n_az))
    pitch = np.deg2rad(np.linspace(float(pitch_deg[0]), float(pitch_deg[1]), beams, dtype=np.float64))
    az = np.deg2rad(float(azimuth_deg[0]) + (np.arange(n_az, dtype=np.float64) + 0.5) * float(azimuth_step_deg))
    b, a = np.meshgrid(np.arange(beams), np.arange(n_az), indexing="ij")
    b, a = b.reshape(-1), a.reshape(-1)
    if tile is not None:
        t = int(tile)
        if t < 1:
            raise ValueError("tile must be >= 1 or None, got %r" % (tile,))
        order = np.lexsort((a % t, b % t, a // t, b // t))        # the last key is the most significant
        b, a = b[order], a[order]
    d = np.stack([np.cos(pitch[b]) * np.cos(az[a]), np.cos(pitch[b]) * np.sin(az[a]), np.sin(pitch[b])], -1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy(d.astype(np.float32))


def sensor_origin(vox_origin, voxel_size):
    """The velodyne origin (0, 0, 0 of the sensor frame) in grid units of a grid that starts at `vox_origin` metres ->
    (3,) float32 tensor.  SemanticKITTI: (0, -25.6, -2) at 0.2 m -> (0, 128, 10)."""
    org = np.asarray(vox_origin, dtype=np.float64).reshape(3)
    return torch.from_numpy(((0.0 - org) / float(voxel_size)).astype(np.float32))


def trajectory_origins(poses, frame, count, step, vox_origin, voxel_size, dims):
    """RayIoU's multi-origin sampling: the sensor positions of frames frame, frame + step, ... of `poses` ({frame: 4 x 4
    sensor -> world}, fuse.read_kitti_poses), expressed in the grid of `frame` -> (K, 3) float32 tensor, 1 <= K <= count.
    At most `count` frames that exist are taken (a missing frame is skipped and does not count; the walk ends with the
    last pose); of those, the positions inside the closed box [0, X] x [0, Y] x [0, Z] are kept.  The frame's own origin
    comes first and is always kept.  Composed in float64 like fuse.grid_affine: T = pose_frame^-1 pose_f, position =
    (t(T) - vox_origin) / voxel_size.  Later positions see surfaces that are hidden from the current one; SemanticKITTI's
    targets are aggregated over later scans, so scoring them is legitimate."""
    from .fuse import _rigid_inverse
    frame, count, step = int(frame), int(count), int(step)
    if count < 1 or step < 1:
        raise ValueError("count and step must be >= 1, got %r, %r" % (count, step))
    if frame not in poses:
        raise KeyError("no pose for frame %d" % frame)
    org = np.asarray(vox_origin, dtype=np.float64).reshape(3)
    hi = np.asarray(dims, dtype=np.float64).reshape(3)
    inv = _rigid_inverse(poses[frame])
    out, taken, f, last = [], 0, frame, max(poses)
    while taken < count and f <= last:
        if f in poses:
            taken += 1
            T = inv @ np.asarray(poses[f], dtype=np.float64)
            g = (T[:3, 3] - org) / float(voxel_size)
            if f == frame:
                g = (0.0 - org) / float(voxel_size)               # exact, whatever the pose
            if f == frame or bool(np.all((g >= 0.0) & (g <= hi))):
                out.append(g)
        f += step
    return torch.from_numpy(np.stack(out).astype(np.float32))


# ----------------------------------------------------------------------------------------------------- the metric
class RayMetrics:
    """The ray-wise counters of RayIoU on the GPU and the statistics made of them.

    n_classes <= 32 (class 0 is free space); voxel_size in metres turns thresholds_m into grid units (float32(m /
    voxel_size), handed to the kernel by value); dirs (N, 3) float32 unit vectors (default: lidar_directions());
    unknown "drop" (default) or "pass".  The counters are one int64 tensor, allocated and zeroed on the device of the first
    batch (outside any capture); add_batch is one launch without host synchronisation."""

    def __init__(self, n_classes, voxel_size, dirs=None, thresholds_m=(1.0, 2.0, 4.0), unknown="drop"):
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= hip.RAY_MAX_CLASSES:
            raise ValueError("n_classes must be 1..%d, got %r" % (hip.RAY_MAX_CLASSES, n_classes))
        self.voxel_size = float(voxel_size)
        if not self.voxel_size > 0.0:
            raise ValueError("voxel_size must be positive, got %r" % (voxel_size,))
        self.thresholds_m = tuple(float(t) for t in thresholds_m)
        if not 1 <= len(self.thresholds_m) <= hip.RAY_MAX_THRESHOLDS or any(not t > 0.0 for t in self.thresholds_m):
            raise ValueError("1..%d positive thresholds (metres), got %r" % (hip.RAY_MAX_THRESHOLDS, thresholds_m))
        if unknown not in UNKNOWN_MODES:
            raise ValueError("unknown is 'drop' or 'pass', got %r" % (unknown,))
        self.unknown = unknown
        self.thresholds = tuple(float(np.float32(t / self.voxel_size)) for t in self.thresholds_m)   # grid units
        dirs = lidar_directions() if dirs is None else torch.as_tensor(np.array(dirs) if isinstance(dirs, np.ndarray) else dirs)
        if dirs.dim() != 2 or dirs.shape[1] != 3 or dirs.shape[0] < 1:
            raise ValueError("dirs must be (N, 3), got %r" % (tuple(dirs.shape),))
        self.dirs = dirs.to(torch.float32).contiguous()
        self.size = hip.ray_metric_size(self.n_classes, len(self.thresholds))
        self._counts = None

    def _alloc(self, device):
        if self._counts is None:
            self._counts = torch.zeros(self.size, dtype=torch.int64, device=device)
        elif self._counts.device != device:
            self._counts = self._counts.to(device)
        if self.dirs.device != device:
            self.dirs = self.dirs.to(device)
        return self._counts

    @staticmethod
    def _labels(t, name):
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("%s must be a (B, X, Y, Z) integer label tensor, got %s %s"
                             % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, getattr(t, "dtype", None)))
        if t.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)):
            t = t.to(torch.int16)                                  # class ids and 255 fit
        return t.contiguous()

    def add_batch(self, pred_labels, target, origins):
        """pred_labels, target (B, X, Y, Z) integer labels on the GPU (1- and 2-byte labels are read in place, wider ones
        narrowed to 2 bytes); origins (B, K, 3), or (K, 3) / (3,) for all frames, grid units.  One launch."""
        pred, target = self._labels(pred_labels, "pred_labels"), self._labels(target, "target")
        if pred.shape != target.shape:
            raise ValueError("pred_labels %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
        B = int(pred.shape[0])
        origins = torch.as_tensor(origins).to(device=pred.device, dtype=torch.float32)
        if origins.dim() <= 2:
            origins = origins.reshape(1, -1, 3).expand(B, -1, 3)
        if origins.dim() != 3 or origins.shape[0] != B or origins.shape[2] != 3 or origins.shape[1] < 1:
            raise ValueError("origins must be (B, K, 3) with B = %d, (K, 3) or (3,), got %r" % (B, tuple(origins.shape)))
        counts = self._alloc(pred.device)
        hip.ray_metric(pred, target.to(pred.device), origins.contiguous(), self.dirs, counts, self.thresholds, self.n_classes,
                       UNKNOWN_MODES[self.unknown])
        return self

    def reset(self):
        if self._counts is not None:
            self._counts.zero_()
        return self

    def counts(self):
        """The int64 counters (a CPU tensor of zeroes before the first batch), in the kernel's layout: rays, valid, unknown,
        pred_miss, gt[C], pred[C], tp[T][C], tp_geo[T]."""
        return torch.zeros(self.size, dtype=torch.int64) if self._counts is None else self._counts

    def merge_(self, other_counts):
        """Add the counters of another RayMetrics (or its counts() tensor), e.g. another rank's."""
        other = other_counts.counts() if isinstance(other_counts, RayMetrics) else torch.as_tensor(other_counts)
        if other.numel() != self.size or other.dtype != torch.int64:
            raise ValueError("merge_ takes %d int64 counters, got %s %s" % (self.size, tuple(other.shape), other.dtype))
        mine = self._alloc(self._counts.device if self._counts is not None else other.device)
        mine += other.reshape(-1).to(mine.device)
        return self

    def allreduce_(self, dist=None):
        """Sum the counters over the ranks of torch.distributed (in place); a no-op without a process group."""
        if dist is None:
            import torch.distributed as dist
            if not dist.is_available():
                return self
        if dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self._alloc(self._counts.device if self._counts is not None
                                        else torch.device("cuda" if torch.cuda.is_available() else "cpu")), op=dist.ReduceOp.SUM)
        return self

    def split(self, counts=None):
        """The counters by name -> {"rays", "valid", "unknown", "pred_miss": int, "gt", "pred": (C,), "tp": (T, C),
        "tp_geo": (T,)} as int64 numpy (one device -> host copy)."""
        c = (self.counts() if counts is None else torch.as_tensor(counts)).detach().cpu().numpy().astype(np.int64).reshape(-1)
        C, T, n = self.n_classes, len(self.thresholds), len(SCALARS)
        out = {name: int(c[i]) for i, name in enumerate(SCALARS)}
        out["gt"], out["pred"] = c[n:n + C].copy(), c[n + C:n + 2 * C].copy()
        out["tp"] = c[n + 2 * C:n + 2 * C + T * C].reshape(T, C).copy()
        out["tp_geo"] = c[n + 2 * C + T * C:n + 2 * C + T * C + T].copy()
        return out

    def get_stats(self):
        """-> ray_iou (T, C) = tp / (gt + pred - tp) per threshold and class (0 where the denominator is 0); ray_miou (T,)
        the mean over the classes 1 .. C - 1 that occur -- a class with gt + pred == 0 (no valid ray hit it in either
        volume) is EXCLUDED from the mean rather than counted as 0, and the mean is 0 when no class occurs; RayIoU their
        mean over the thresholds; ray_iou_geo (T,) = tp_geo / (valid + pred_hits - tp_geo), pred_hits = valid - pred_miss,
        the class-agnostic score; thresholds_m; and the raw tallies (rays, valid, unknown, pred_miss, gt, pred, tp,
        tp_geo).  The divisions are float64 on the host."""
        s = self.split()
        gt, pred, tp = s["gt"].astype(np.float64), s["pred"].astype(np.float64), s["tp"].astype(np.float64)
        den = gt[None] + pred[None] - tp
        iou = np.divide(tp, den, out=np.zeros_like(tp), where=den > 0)
        seen = (gt + pred) > 0
        seen[0] = False
        miou = iou[:, seen].mean(1) if seen.any() else np.zeros(len(self.thresholds))
        geo = s["tp_geo"].astype(np.float64)
        gden = float(s["valid"]) + float(s["valid"] - s["pred_miss"]) - geo
        out = dict(s)
        out.update({"ray_iou": iou, "ray_miou": miou, "RayIoU": float(miou.mean()),
                    "ray_iou_geo": np.divide(geo, gden, out=np.zeros_like(geo), where=gden > 0),
                    "thresholds_m": self.thresholds_m})
        return out


def format_report(stats, class_names, prefix):
    """The printed block of a RayMetrics.get_stats(): the `<prefix>======` line, the scores per threshold, the per-class
    table and the ray tallies -> list of lines."""
    thr = stats["thresholds_m"]
    lines = ["{}======".format(prefix),
             "RayIoU={:.4f}, ".format(stats["RayIoU"] * 100)
             + ", ".join("RayIoU@{:g}={:.4f}".format(t, v * 100) for t, v in zip(thr, stats["ray_miou"]))
             + ", RayIoU_geo={:.4f}".format(float(np.mean(stats["ray_iou_geo"])) * 100),
             "class RayIoU: {}, ".format(list(class_names))]
    for t, row in zip(thr, stats["ray_iou"]):
        lines.append("@{:g}m: ".format(t) + " ".join("{:.4f}, ".format(v * 100) for v in row.tolist()))
    lines.append("rays={}, valid={}, unknown={}, pred_miss={}".format(stats["rays"], stats["valid"], stats["unknown"],
                                                                     stats["pred_miss"]))
    return lines
