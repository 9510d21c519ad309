"""Distance-tolerant scores: precision, recall and F-score at a distance and the Chamfer distance between predicted and
true occupied voxels, class-agnostic and per class (K37, csrc/edt.hip).

Voxel IoU counts a pole predicted one voxel to the side as a complete miss and a complete false alarm; RayIoU forgives that
only along the rays of one sensor position.  The usual complement -- what the surround-view occupancy benchmarks report
beside mIoU -- asks how far off the geometry is: for every predicted occupied voxel the distance to the nearest true one
(precision side) and for every true one the distance to the nearest predicted one (recall side).  All of it is a function
of one primitive, the exact Euclidean distance transform of a label volume, whose squared values on a voxel grid are
integers: `hip.edt_sq` computes it and `hip.dist_metric` turns it into histograms without leaving the GPU.

    m = DistanceMetrics(20, 0.2)                      # thresholds 0.2 / 0.4 / 0.8 m, distances truncated at max_d2 = 1024
    m.add_batch(pred_labels, target)                  # counters and scratch stay on the GPU, no host sync
    s = m.get_stats()
    s["F_geo"], s["F_sem"], s["CD_geo"], s["CD_sem"]

Definitions (include/occdepth_amd.h has the contract).  Classes are 0 .. C - 1, 0 free.  Slot 0 of a volume is every voxel
with 1 <= label < C, slot c >= 1 every voxel with label == c; labels >= C (255 included) are never seeds.  D_s(v) =
min(squared distance in voxels from v to the nearest seed of slot s, T + 1), T = max_d2.  A voxel is a query iff target !=
255 (and mask != 0 with a mask); seeds are NOT masked.  counts[0][s][d]: prediction voxels of slot s (queries) at squared
distance d from the target's slot s; counts[1][s][d]: target voxels of slot s at squared distance d from the prediction's.
Bin T + 1 is "further than T or nothing there".

`edt_sq_ref` and `dist_metric_ref` restate both kernels in numpy; the GPU tests hold the kernels to them with exact
equality.  No score of a trained model was computed where this was built (no checkpoint and no dataset): the module
delivers the metric, pinned against its restatement, and its cost.
"""
import numpy as np
import torch

from . import hip


# ----------------------------------------------------------------------------------------------------- numpy restatements
def _as_labels(vol):
    a = vol.detach().cpu().numpy() if torch.is_tensor(vol) else np.asarray(vol)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    return a.astype(np.int64)


def seeds_of(labels, slot, n_classes):
    """The seed set of a slot -> bool array of labels' shape."""
    labels = np.asarray(labels)
    return ((labels >= 1) & (labels < n_classes)) if slot == 0 else (labels == slot)


def _min_plus(g, axis, r, cap):
    """out[i] = min(min over |k| <= r of g[i + k] + k^2, cap) along `axis` (int64)."""
    n = g.shape[axis]
    out = g.copy()
    for k in range(1, min(r, n - 1) + 1):
        lo = [slice(None)] * g.ndim
        hi = [slice(None)] * g.ndim
        lo[axis], hi[axis] = slice(0, n - k), slice(k, n)
        lo, hi = tuple(lo), tuple(hi)
        out[lo] = np.minimum(out[lo], g[hi] + k * k)
        out[hi] = np.minimum(out[hi], g[lo] + k * k)
    return np.minimum(out, cap)


def edt_sq_ref(labels, slots, n_classes, max_d2):
    """labels (B, X, Y, Z) integer array -> (B, len(slots), X, Y, Z) uint16: the separable definition, pass by pass along
    z, y and x with the window floor(sqrt(max_d2)) and the clip at max_d2 + 1 after every pass."""
    labels = _as_labels(labels)
    T = int(max_d2)
    r = int(np.floor(np.sqrt(T)))
    while (r + 1) * (r + 1) <= T:
        r += 1
    while r * r > T:
        r -= 1
    B = labels.shape[0]
    out = np.empty((B, len(slots)) + labels.shape[1:], dtype=np.uint16)
    for i, s in enumerate(slots):
        g = np.where(seeds_of(labels, int(s), n_classes), 0, T + 1).astype(np.int64)
        for axis in (3, 2, 1):
            g = _min_plus(g, axis, r, T + 1)
        out[:, i] = g
    return out


def dist_metric_ref(pred, target, mask, n_classes, max_d2):
    """The counters of occd_dist_metric in its layout -> (2 C (T + 2),) int64."""
    pred, target = _as_labels(pred), _as_labels(target)
    C, T = int(n_classes), int(max_d2)
    query = target != 255
    if mask is not None:
        m = mask.detach().cpu().numpy() if torch.is_tensor(mask) else np.asarray(mask)
        query &= m.astype(bool)
    counts = np.zeros((2, C, T + 2), dtype=np.int64)
    slots = list(range(C))
    for side, (members, seeds) in enumerate(((pred, target), (target, pred))):
        D = edt_sq_ref(seeds, slots, C, T)
        for s in slots:
            sel = query & seeds_of(members, s, C)
            counts[side, s] += np.bincount(D[:, s][sel].astype(np.int64), minlength=T + 2)
    return counts.reshape(-1)


def threshold_bins(thresholds_m, voxel_size, max_d2):
    """Metres -> the largest squared voxel distance that still counts: k = floor((tau / voxel_size)^2 + 1e-6); 1, 4, 16 for
    0.2 / 0.4 / 0.8 m at 0.2 m.  Refused when k > max_d2 (the histogram does not resolve it)."""
    out = []
    for tau in thresholds_m:
        k = int(np.floor((float(tau) / float(voxel_size)) ** 2 + 1e-6))
        if k > int(max_d2):
            raise ValueError("threshold %g m is %d in squared voxels, past max_d2 = %d" % (tau, k, max_d2))
        out.append(k)
    return tuple(out)


# ----------------------------------------------------------------------------------------------------- the metric
class DistanceMetrics:
    """The distance histograms on the GPU and the statistics made of them.

    n_classes <= 32 (class 0 is free space); voxel_size in metres; thresholds_m: distances at which precision / recall / F
    are reported; max_d2 (1 .. 65534): squared voxel distances are truncated at max_d2 + 1, so the Chamfer distance is
    truncated at voxel_size * sqrt(max_d2 + 1) -- 6.4 m at the defaults.  The counters (2 C (max_d2 + 2) int64) and the
    scratch (hip.dist_metric_scratch_bytes(dims) = 32 X Y Z bytes, 64 MiB at 256 x 256 x 32, whatever the batch size) are
    allocated on the device of the first batch, outside any capture; add_batch is one call without host synchronisation."""

    def __init__(self, n_classes, voxel_size, thresholds_m=(0.2, 0.4, 0.8), max_d2=1024):
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= hip.EDT_MAX_CLASSES:
            raise ValueError("n_classes must be 1..%d, got %r" % (hip.EDT_MAX_CLASSES, n_classes))
        self.voxel_size = float(voxel_size)
        if not self.voxel_size > 0.0:
            raise ValueError("voxel_size must be positive, got %r" % (voxel_size,))
        self.max_d2 = int(max_d2)
        if not 1 <= self.max_d2 <= hip.EDT_MAX_D2:
            raise ValueError("max_d2 must be 1..%d, got %r" % (hip.EDT_MAX_D2, max_d2))
        self.thresholds_m = tuple(float(t) for t in thresholds_m)
        if not self.thresholds_m or any(not t > 0.0 for t in self.thresholds_m):
            raise ValueError("at least one positive threshold (metres), got %r" % (thresholds_m,))
        self.bins = threshold_bins(self.thresholds_m, self.voxel_size, self.max_d2)
        self.size = hip.dist_metric_size(self.n_classes, self.max_d2)
        self._counts = None
        self._scratch = None

    def scratch_bytes(self):
        """Bytes of the scratch buffer this object holds (0 before the first batch)."""
        return 0 if self._scratch is None else int(self._scratch.numel())

    def _alloc(self, device, dims=None):
        if self._counts is None:
            self._counts = torch.zeros(self.size, dtype=torch.int64, device=device)
        elif self._counts.device != device:
            self._counts = self._counts.to(device)
        if dims is not None:
            need = hip.dist_metric_scratch_bytes(dims)
            if self._scratch is None or self._scratch.numel() < need or self._scratch.device != device:
                self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        return self._counts

    @staticmethod
    def _labels(t, name):
        if not torch.is_tensor(t) or t.dim() != 4 or t.dtype.is_floating_point or t.dtype == torch.bool:
            raise ValueError("%s must be a (B, X, Y, Z) integer label tensor, got %s %s"
                             % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, getattr(t, "dtype", None)))
        if t.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)):
            t = t.to(torch.int16)                                  # class ids and 255 fit
        return t.contiguous()

    def add_batch(self, pred_labels, target, mask=None):
        """pred_labels, target (B, X, Y, Z) integer labels on the GPU (1- and 2-byte labels are read in place, wider ones
        narrowed to 2 bytes); mask None or (B, X, Y, Z) bool / uint8: the voxels that may be queries."""
        pred, target = self._labels(pred_labels, "pred_labels"), self._labels(target, "target")
        if pred.shape != target.shape:
            raise ValueError("pred_labels %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
        if mask is not None:
            if not torch.is_tensor(mask) or mask.numel() != pred.numel() or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("mask must be a bool / uint8 tensor of pred_labels' size %s, got %s %s"
                                 % (tuple(pred.shape), tuple(mask.shape) if torch.is_tensor(mask) else type(mask).__name__,
                                    getattr(mask, "dtype", None)))
            mask = mask.reshape(pred.shape).to(pred.device).contiguous()
        counts = self._alloc(pred.device, tuple(pred.shape[1:]))
        hip.dist_metric(pred, target.to(pred.device), counts, self.n_classes, self.max_d2, self._scratch, mask)
        return self

    def reset(self):
        if self._counts is not None:
            self._counts.zero_()
        return self

    def counts(self):
        """The int64 counters (a CPU tensor of zeroes before the first batch), in the kernel's layout [2][C][max_d2 + 2]."""
        return torch.zeros(self.size, dtype=torch.int64) if self._counts is None else self._counts

    def merge_(self, other_counts):
        """Add the counters of another DistanceMetrics (or its counts() tensor), e.g. another rank's."""
        other = other_counts.counts() if isinstance(other_counts, DistanceMetrics) else torch.as_tensor(other_counts)
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

    def get_stats(self):
        """From the counters alone, in float64 on the host (one device -> host copy).  With c = counts[side][slot] and k the
        integer of a threshold: precision = sum(c[0][s][:k + 1]) / sum(c[0][s]), recall the same on side 1 (0 where the
        side is empty), F = 2 P R / (P + R) (0 when both are 0).  ->
          precision, recall, F            (n_thresholds, C): row per threshold, column per slot (column 0 class-agnostic)
          precision_geo, recall_geo, F_geo  (n_thresholds,): slot 0
          F_sem                           (n_thresholds,): the mean of F over the classes c >= 1 with a target query
          CD (C,), CD_geo, CD_sem         the truncated Chamfer distance in metres: voxel_size * (mean over side 0 of
                                          sqrt(bin) + mean over side 1 of sqrt(bin)); a side without a query adds 0; bin
                                          max_d2 + 1 counts as sqrt(max_d2 + 1), so CD is TRUNCATED at voxel_size *
                                          sqrt(max_d2 + 1) per side (6.4 m at the defaults); CD_sem is the mean over the
                                          classes c >= 1 with a target query
          overflow (2, C), overflow_geo (2,)  the share of each side's queries in bin max_d2 + 1 (what the truncation hid)
          queries (2, C)                  the number of queries per side and slot
          thresholds_m, bins, present     the thresholds, their integers, the classes c >= 1 with a target query."""
        C, T = self.n_classes, self.max_d2
        c = self.counts().detach().cpu().numpy().astype(np.float64).reshape(2, C, T + 2)
        total = c.sum(2)                                                        # (2, C)
        safe = np.where(total > 0, total, 1.0)
        within = np.stack([c[:, :, :k + 1].sum(2) / safe for k in self.bins])   # (n_thresholds, 2, C)
        P, R = within[:, 0], within[:, 1]
        F = np.divide(2 * P * R, P + R, out=np.zeros_like(P), where=(P + R) > 0)
        root = np.sqrt(np.arange(T + 2, dtype=np.float64))
        mean_d = (c * root).sum(2) / safe                                       # (2, C) voxels
        CD = self.voxel_size * (mean_d[0] + mean_d[1])
        present = total[1] > 0
        present[0] = False
        overflow = c[:, :, T + 1] / safe
        n = int(present.sum())
        return {"precision": P, "recall": R, "F": F, "precision_geo": P[:, 0], "recall_geo": R[:, 0], "F_geo": F[:, 0],
                "F_sem": F[:, present].mean(1) if n else np.zeros(len(self.bins)),
                "CD": CD, "CD_geo": float(CD[0]), "CD_sem": float(CD[present].mean()) if n else 0.0,
                "overflow": overflow, "overflow_geo": overflow[:, 0], "queries": total.astype(np.int64),
                "thresholds_m": self.thresholds_m, "bins": self.bins, "present": present,
                "truncation_m": self.voxel_size * float(np.sqrt(T + 1))}


def format_report(stats, class_names, prefix):
    """The printed block of a DistanceMetrics.get_stats(): the `<prefix>======` line, the class-agnostic and the semantic
    scores per threshold, the Chamfer distances with the share of queries the truncation hid, and the per-class table ->
    list of lines."""
    thr = stats["thresholds_m"]
    lines = ["{}======".format(prefix)]
    for i, t in enumerate(thr):
        lines.append("@{:g}m: F_geo={:.4f}, Precision_geo={:.4f}, Recall_geo={:.4f}, F_sem={:.4f}".format(
            t, stats["F_geo"][i] * 100, stats["precision_geo"][i] * 100, stats["recall_geo"][i] * 100, stats["F_sem"][i] * 100))
    lines.append("CD_geo={:.4f} m, CD_sem={:.4f} m (truncated at {:.2f} m per side; beyond it: {:.2f} % of the predicted, "
                 "{:.2f} % of the true occupied voxels)".format(stats["CD_geo"], stats["CD_sem"], stats["truncation_m"],
                                                                stats["overflow_geo"][0] * 100, stats["overflow_geo"][1] * 100))
    lines.append("class F / CD: {}, ".format(list(class_names)))
    for i, t in enumerate(thr):
        lines.append("F@{:g}m: ".format(t) + " ".join("{:.4f}, ".format(v * 100) for v in stats["F"][i].tolist()))
    lines.append("CD[m]: " + " ".join("{:.4f}, ".format(v) for v in stats["CD"].tolist()))
    return lines
