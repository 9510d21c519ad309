"""SSC metrics, mirror of occdepth/loss/sscMetrics.py (SSCMetrics.add_batch / get_stats / reset).

The reference pulls the logits to the host every step (OccDepth.py:523-526: `.cpu().numpy()`, np.argmax) and
counts tp/fp/fn with numpy `where` per class.  Here the arg-max and the counting are one HIP pass (K7,
csrc/loss.hip) into a (C, C) int64 confusion matrix that stays on the GPU; nothing synchronises until
`get_stats()`.  All counters of the reference derive from that matrix:
    tps[j] = hist[j, j]   fps[j] = sum_t hist[t, j] - tps[j]   fns[j] = sum_p hist[j, p] - tps[j]
    completion (occupied = label > 0): tp = hist[1:, 1:].sum(), fp = hist[0, 1:].sum(), fn = hist[1:, 0].sum()

Metrics by region (`regions=`): the same pass counts every voxel into all the regions it belongs to -- an index box, the
camera field of view, byte masks -- as one (R, C, C) `region_hist` (hip.ssc_confusion_regions), optionally per frame.
The reference's `nonempty` / `nonsurface` masks (sscMetrics.py:70-91, the SSCNet / NYU protocol) are two such regions.
"""
import numpy as np
import torch

from .. import hip


class Region:
    """One evaluation region: `box` = (x0, x1, y0, y1, z0, z1) voxel indices, half open (None: the whole grid; see
    `metric_box` for metres), `fov`: only voxels inside the camera field of view, `masks`: indices of the masks passed
    to `add_batch(..., masks=)` that must all be non-zero."""

    __slots__ = ("name", "box", "fov", "masks")

    def __init__(self, name, box=None, fov=False, masks=()):
        self.name = str(name)
        self.box = None if box is None else tuple(int(v) for v in box)
        self.fov = bool(fov)
        self.masks = tuple(int(m) for m in masks)
        if self.box is not None and len(self.box) != 6:
            raise ValueError("a region box is (x0, x1, y0, y1, z0, z1)")
        if any(not 0 <= m < 3 for m in self.masks):
            raise ValueError("a region names mask slots 0..2")

    @property
    def need(self):
        return (hip.NEED_FOV if self.fov else 0) | sum({hip.NEED_MASK0 << m for m in self.masks})

    def __repr__(self):
        return "Region(%r, box=%r, fov=%r, masks=%r)" % (self.name, self.box, self.fov, self.masks)


def metric_box(box_m, vox_origin, voxel_size, grid):
    """(x0, x1, y0, y1[, z0, z1]) in metres (sensor frame; all z when left out) -> the index box of a `Region` on a grid of
    `grid` = (X, Y, Z) voxels of `voxel_size` metres from `vox_origin`: every bound goes to the nearest voxel edge and is
    clipped to the grid.  ValueError when nothing is left."""
    if len(box_m) not in (4, 6):
        raise ValueError("a metric box is (x0, x1, y0, y1[, z0, z1])")
    out = []
    for ax in range(3):
        if 2 * ax >= len(box_m):
            out += [0, int(grid[ax])]
            continue
        lo, hi = (int(np.floor((float(m) - float(vox_origin[ax])) / float(voxel_size) + 0.5)) for m in box_m[2 * ax:2 * ax + 2])
        lo, hi = max(lo, 0), min(hi, int(grid[ax]))
        if lo >= hi:
            raise ValueError("metric box %r leaves no voxel of the %r grid (axis %d)" % (tuple(box_m), tuple(grid), ax))
        out += [lo, hi]
    return tuple(out)


def stats_from_hist(h):
    """The reference's five statistics (sscMetrics.py:93-109) from one (C, C) confusion matrix [target, prediction]."""
    h = np.asarray(h, dtype=np.float64)
    tps = np.diag(h).copy()
    fps, fns = h.sum(0) - tps, h.sum(1) - tps
    return _stats(h, tps, fps, fns)


def _stats(h_completion, tps, fps, fns):
    h = h_completion
    c_tp, c_fp, c_fn = h[1:, 1:].sum(), h[0, 1:].sum(), h[1:, 0].sum()
    if c_tp != 0:
        precision = c_tp / (c_tp + c_fp)
        recall = c_tp / (c_tp + c_fn)
        iou = c_tp / (c_tp + c_fp + c_fn)
    else:
        precision, recall, iou = 0, 0, 0
    iou_ssc = tps / (tps + fps + fns + 1e-5)
    return {"precision": precision, "recall": recall, "iou": iou, "iou_ssc": iou_ssc,
            "iou_ssc_mean": np.mean(iou_ssc[1:])}


# the reference's add_batch(nonempty=, nonsurface=): completion under labelled & nonempty & nonsurface, classes under
# labelled & nonempty; the masks given fill the slots in this order
_MASKED = ("nonempty", "nonsurface")


class SSCMetrics:
    def __init__(self, n_classes, device=None, regions=None, per_frame=False):
        self.n_classes = n_classes
        self.device = torch.device(device) if device is not None else None   # None: wherever the first batch lives
        self.regions = None if regions is None else tuple(regions)
        self.per_frame = bool(per_frame)
        if self.regions is not None:
            if not 1 <= len(self.regions) <= hip.MAX_REGIONS:
                raise ValueError("1..%d regions per metric object" % hip.MAX_REGIONS)
            if len({r.name for r in self.regions}) != len(self.regions):
                raise ValueError("region names must be unique")
        elif self.per_frame:
            raise ValueError("per_frame needs regions")
        self.reset()

    def reset(self):
        # The matrix is allocated with the first batch (the model is built before .to(device)) and from then on zeroed
        # IN PLACE: a captured training-step hipGraph (train_graph.py) keeps accumulating into this very buffer, so
        # replacing the tensor would leave the replays counting into an orphan and `get_stats()` reading zeros.
        hist = self.__dict__.get("hist")
        if hist is not None:
            hist.zero_()
        else:
            self.hist = None
        for name in ("region_hist", "masked_hist"):       # (R, C, C) by region / (2, C, C) of the masked form: same rule
            h = self.__dict__.get(name)
            if h is not None:
                h.zero_()
            else:
                setattr(self, name, None)
        self.frame_hists = []         # per_frame: one (B, R, C, C) device tensor per batch
        self._form = None             # "plain" / "masked": which form of add_batch this object has seen since reset()
        self.count = 1e-8

    def _alloc(self, device):
        if self.hist is None:
            self.hist = torch.zeros(self.n_classes, self.n_classes, dtype=torch.int64,
                                    device=self.device if self.device is not None else device)
        return self.hist

    def _u8(self, a, device):
        t = torch.as_tensor(a)
        return t.to(device=device, dtype=torch.uint8).contiguous()

    def _alloc_n(self, name, n, device):
        h = getattr(self, name)
        if h is None:
            h = torch.zeros(n, self.n_classes, self.n_classes, dtype=torch.int64,
                            device=self.device if self.device is not None else device)
            setattr(self, name, h)
        return h

    def _mask(self, a, like):
        """bool / uint8, numpy or torch, (B, X, Y, Z) or (B, N) -> a device mask shaped like the target (bool stays bool:
        the binding passes its uint8 view, no copy)."""
        t = torch.as_tensor(a)
        if t.dtype not in (torch.bool, torch.uint8):
            t = t != 0
        return t.to(like.device).reshape(like.shape).contiguous()

    def _set_form(self, form):
        if self._form is not None and self._form != form:
            raise RuntimeError("this SSCMetrics object has counted %s batches since its last reset(): the nonempty / "
                               "nonsurface form and the unmasked form do not share counters" % self._form)
        self._form = form

    def _device_for(self, y_true):
        if self.device is not None:
            return self.device
        return y_true.device if torch.is_tensor(y_true) and y_true.is_cuda else \
            torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def _add_regions(self, target, fov, masks, **pred):
        """One launch: every region of the object, shared matrices (+ one block per frame with per_frame)."""
        R = len(self.regions)
        if any(r.fov for r in self.regions) and fov is None:
            raise ValueError("a region of this metric needs the camera FOV: pass fov= (a mask or the calibration tuple)")
        n_masks = 1 + max((m for r in self.regions for m in r.masks), default=-1)
        if len(masks) < n_masks:
            raise ValueError("the regions of this metric use %d mask(s), got %d" % (n_masks, len(masks)))
        masks = tuple(self._mask(m, target) for m in masks)
        if torch.is_tensor(fov) or isinstance(fov, np.ndarray):
            fov = self._mask(fov, target)
        desc = [(r.box, r.need) for r in self.regions]
        hist = self._alloc_n("region_hist", R, target.device)
        if self.per_frame:
            blk = torch.zeros((target.shape[0], R) + tuple(hist.shape[1:]), dtype=torch.int64, device=hist.device)
            hip.ssc_confusion_regions(blk, target, desc, masks=masks, fov=fov, per_frame=True, **pred)
            hist.add_(blk.sum(0))
            self.frame_hists.append(blk)
        else:
            hip.ssc_confusion_regions(hist, target, desc, masks=masks, fov=fov, **pred)

    def add_batch(self, y_pred, y_true, nonempty=None, nonsurface=None, fov=None, masks=()):
        """y_pred / y_true: (B, X, Y, Z) class volumes (numpy or torch), 255 = unlabelled in y_true.  nonempty /
        nonsurface: the reference's masks (bool or uint8, numpy or torch, (B, X, Y, Z) or (B, N)).  With `regions`:
        fov (a mask, or the calibration tuple of hip.ssc_confusion_regions) and the masks the regions name."""
        masked = nonempty is not None or nonsurface is not None
        if self.regions is not None:
            if masked:
                raise ValueError("a metric with regions takes its masks through Region(masks=...) and masks=")
            self.count += 1
            dev = self._device_for(y_true)
            self._add_regions(self._u8(y_true, dev), fov, masks, labels=self._u8(y_pred, dev))
            return
        if fov is not None or len(masks):
            raise ValueError("fov= / masks= need a metric constructed with regions")
        self._set_form("masked" if masked else "plain")
        self.count += 1
        dev = self._device_for(y_true)
        if masked:
            hist = self._alloc_n("masked_hist", 2, dev)
            target = self._u8(y_true, hist.device)
            given = [m for m in (nonempty, nonsurface) if m is not None]
            both = sum({hip.NEED_MASK0 << i for i in range(len(given))})
            classes = hip.NEED_MASK0 if nonempty is not None else 0
            hip.ssc_confusion_regions(hist, target, [(None, both), (None, classes)],
                                      labels=self._u8(y_pred, hist.device), masks=[self._mask(m, target) for m in given])
            return
        hist = self._alloc(dev)
        hip.ssc_confusion(hist, self._u8(y_true, hist.device), labels=self._u8(y_pred, hist.device))

    def add_batch_logits(self, ssc_logit, y_true, fov=None, masks=()):
        """Fused variant of the step's `np.argmax(ssc_pred) -> add_batch`: logits (B, C, X, Y, Z) on the GPU."""
        if self.regions is not None:
            self.count += 1
            self._add_regions(self._u8(y_true, ssc_logit.device), fov, masks, logits=ssc_logit.detach().float())
            return
        if fov is not None or len(masks):
            raise ValueError("fov= / masks= need a metric constructed with regions")
        self._set_form("plain")
        self.count += 1
        hist = self._alloc(ssc_logit.device)
        hip.ssc_confusion(hist, self._u8(y_true, hist.device), logits=ssc_logit.detach().float())     # (planes or channels-last rows: read in place)

    # -- host-side views (synchronise) ----------------------------------------------------------------------
    def _counts(self):
        """(matrix the completion counts come from, tps, fps, fns).  After the masked form of add_batch the completion
        matrix is the one counted under nonempty & nonsurface and the class counters come from the nonempty one."""
        if self._form == "masked" and self.masked_hist is not None:
            both, h = self.masked_hist.cpu().numpy().astype(np.float64)
        elif self.hist is None:
            both = h = np.zeros((self.n_classes, self.n_classes), dtype=np.float64)
        else:
            both = h = self.hist.cpu().numpy().astype(np.float64)
        tps = np.diag(h).copy()
        return both, tps, h.sum(0) - tps, h.sum(1) - tps

    def _region_index(self, region):
        if self.regions is None:
            raise ValueError("this metric was constructed without regions")
        names = [r.name for r in self.regions]
        if isinstance(region, Region):
            region = region.name
        if isinstance(region, str):
            if region not in names:
                raise KeyError("no region %r (have %s)" % (region, names))
            return names.index(region)
        return range(len(names))[region]

    def _region_counts(self):
        if self.region_hist is None:
            return np.zeros((len(self.regions), self.n_classes, self.n_classes), dtype=np.float64)
        return self.region_hist.cpu().numpy().astype(np.float64)

    def get_region_stats(self):
        """name -> the reference's five statistics on that region's matrix (one device-to-host copy)."""
        h = self._region_counts()
        return {r.name: stats_from_hist(h[i]) for i, r in enumerate(self.regions)}

    def frame_stats(self):
        """per_frame: one {region name: statistics} dict per frame counted since reset(), in the order the frames
        arrived.  The only place of the per-frame path that synchronises."""
        if not self.frame_hists:
            return []
        h = torch.cat(self.frame_hists).cpu().numpy().astype(np.float64)
        return [{r.name: stats_from_hist(f[i]) for i, r in enumerate(self.regions)} for f in h]

    @property
    def tps(self):
        return self._counts()[1]

    @property
    def fps(self):
        return self._counts()[2]

    @property
    def fns(self):
        return self._counts()[3]

    def get_stats(self, region=None):
        """The reference's statistics; `region` (name, index or Region) reads that region's matrix instead of `hist`."""
        if region is not None:
            i = self._region_index(region)
            return stats_from_hist(self._region_counts()[i])
        return _stats(*self._counts())

    def merge_(self, other_hist):
        """Add another rank's confusion matrix (after an all-reduce / gather)."""
        self._alloc(other_hist.device).add_(other_hist.to(self.hist.device))
        return self
