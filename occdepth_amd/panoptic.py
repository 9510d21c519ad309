"""Objects in the volumes: connected components of a label volume on the GPU (K40, csrc/ccl.hip), panoptic quality built on
them, and the removal of small components.

Every other score of this project sees a prediction voxel by voxel or ray by ray; voxel mIoU cannot tell one merged blob of
three cars from three cars.  Panoptic scene completion (PaSCo, Cao et al., CVPR 2024) asks for PQ / SQ / RQ: segments of
the prediction are matched to segments of the target, and a class scores by how many of its objects were found and how well.

    m = PanopticMetrics(20, KITTI_THINGS, KITTI_STUFF)
    m.add_batch(pred_labels, target)                  # components, overlaps and their sort on the GPU; matching on the host
    s = m.get_stats()
    s["PQ"], s["PQ_things"], s["PQ_stuff"], s["SQ"], s["RQ"], s["PQ_dagger"]

Definitions (include/occdepth_amd.h has the kernels' contract).  `things` classes: a segment is a maximal set of voxels of
one class connected under `connectivity` (6 or 26).  `stuff` classes: all voxels of the class in a frame are one segment.
Every other label (0 and 255 too) belongs to no segment.  The TARGET's "instances" are therefore connected components of
the target -- a stand-in for the instance annotation that SemanticKITTI's completion volumes do not carry -- unless the
caller passes `target_instances`.  Prediction components are found on the whole prediction (after the min_pred_voxels
filter): an object is not cut by an unknown region.  A voxel is valid iff target != 255 (and mask != 0 with a mask); sizes
and intersections count valid voxels only, and a segment without a valid voxel is ignored.  Per frame and class, g and p
match iff 2 |g n p| > |g| + |p| - |g n p| (IoU > 1/2 as an integer comparison; at most one p per g and one g per p).

`segments_ref`, `compact_ref`, `filter_ref`, `overlaps_ref` and `panoptic_ref` restate the kernels and the metric in numpy;
the GPU tests hold the kernels to them with exact equality.  No PQ of a trained model was computed where this was built (no
checkpoint and no dataset): the module delivers the metric, pinned against its restatement, and its cost.
"""
import numpy as np
import torch

from . import hip

KITTI_THINGS = tuple(range(1, 9))        # car, bicycle, motorcycle, truck, other-vehicle, person, bicyclist, motorcyclist
KITTI_STUFF = tuple(range(9, 20))        # road ... traffic-sign
NYU_THINGS = tuple(range(5, 12))         # chair, bed, sofa, table, tvs, furniture, objects
NYU_STUFF = tuple(range(1, 5))           # ceiling, floor, wall, window

TP, FP, FN, N_PRED, N_GT, N_DAGGER = range(6)   # rows of PanopticMetrics.counts()


def default_classes(dataset):
    """(things, stuff) of a dataset name of the model ("kitti", "NYU")."""
    if str(dataset).lower() == "kitti":
        return KITTI_THINGS, KITTI_STUFF
    if str(dataset).lower() == "nyu":
        return NYU_THINGS, NYU_STUFF
    raise ValueError("no default things / stuff classes for dataset %r: pass them" % (dataset,))


# ----------------------------------------------------------------------------------------------------- numpy restatements
def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _back_offsets(connectivity):
    if int(connectivity) not in (6, 26):
        raise ValueError("connectivity must be 6 or 26, got %r" % (connectivity,))
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) < (0, 0, 0) and (int(connectivity) == 26 or abs(dx) + abs(dy) + abs(dz) == 1):
                    out.append((dx, dy, dz))
    return out


def _side(n, d):
    """(slice of the voxels, slice of their neighbours at offset d) along an axis of n."""
    return (slice(1, n), slice(0, n - 1)) if d < 0 else (slice(0, n - 1), slice(1, n)) if d > 0 else (slice(None), slice(None))


def segments_ref(labels, things, stuff=(), connectivity=26):
    """labels (B, X, Y, Z) integer array -> seg (B, X, Y, Z) int32: 0 outside every segment, else 1 + the smallest
    frame-linear index of the voxel's segment.  Per frame, a union-find over the list of neighbouring things voxels of one
    class, a round at a time: every pair whose roots differ lowers the larger root's parent to the smaller root, then
    every voxel is pointed at its root; until no pair has two roots.  A root is the smallest index of its tree."""
    labels = _np(labels).astype(np.int64)
    things, stuff = sorted(set(int(c) for c in things)), sorted(set(int(c) for c in stuff))
    if set(things) & set(stuff):
        raise ValueError("things and stuff overlap")
    B, X, Y, Z = labels.shape
    N = X * Y * Z
    offs = _back_offsets(connectivity)
    seg = np.zeros((B, X, Y, Z), dtype=np.int32)
    for b in range(B):
        lab = labels[b]
        isthing = np.isin(lab, things)
        index = np.arange(N, dtype=np.int64).reshape(X, Y, Z)
        us, vs = [], []
        for d in offs:
            sv, sn = zip(*(_side(n, k) for n, k in zip((X, Y, Z), d)))
            same = isthing[sv] & isthing[sn] & (lab[sv] == lab[sn])
            us.append(index[sv][same])
            vs.append(index[sn][same])
        u, v = np.concatenate(us), np.concatenate(vs)
        L = np.arange(N, dtype=np.int64)
        for _ in range(N + 1):
            ru, rv = L[u], L[v]
            hi, lo = np.maximum(ru, rv), np.minimum(ru, rv)
            live = hi != lo
            if not live.any():
                break
            np.minimum.at(L, hi[live], lo[live])
            while True:
                nxt = L[L]
                if np.array_equal(nxt, L):
                    break
                L = nxt
        out = np.where(isthing, L.reshape(X, Y, Z) + 1, 0)
        for c in stuff:
            sel = lab == c
            if sel.any():
                out = np.where(sel, int(np.flatnonzero(sel.reshape(-1))[0]) + 1, out)
        seg[b] = out
    return seg


def instance_segments_ref(labels, instances, things, stuff=()):
    """The segments when the things are given by instance ids (1 .. N - 1; other ids belong to no segment)."""
    labels, inst = _np(labels).astype(np.int64), _np(instances).astype(np.int64)
    B = labels.shape[0]
    N = labels[0].size
    seg = np.zeros(labels.shape, dtype=np.int32)
    for b in range(B):
        lab, ins, out = labels[b].reshape(-1), inst[b].reshape(-1), np.zeros(N, dtype=np.int64)
        sel = np.isin(lab, sorted(things)) & (ins >= 1) & (ins < N)
        for i in np.unique(ins[sel]):
            where = np.flatnonzero(sel & (ins == i))
            if len(set(lab[where].tolist())) != 1:
                raise ValueError("instance id %d carries more than one class" % i)
            out[where] = where[0] + 1
        for c in stuff:
            where = np.flatnonzero(lab == c)
            if where.size:
                out[where] = where[0] + 1
        seg[b] = out.reshape(labels.shape[1:])
    return seg


def compact_ref(seg, labels):
    """-> ids (B, X, Y, Z) int32 (segments 1 .. K_b in ascending order of seg, 0 kept), count (B,) int64, and the tables of
    sum(count) rows, frame after frame: seg_class uint8, seg_size int32, seg_index int32."""
    seg, labels = _np(seg).astype(np.int64), _np(labels)
    B = seg.shape[0]
    ids = np.zeros(seg.shape, dtype=np.int32)
    count = np.zeros(B, dtype=np.int64)
    cls, size, index = [], [], []
    for b in range(B):
        s, lab = seg[b].reshape(-1), labels[b].reshape(-1)
        values, inverse, n = np.unique(s, return_inverse=True, return_counts=True)
        first = 1 if values.size and values[0] == 0 else 0
        ids[b] = (inverse.reshape(-1) + (1 - first)).reshape(seg.shape[1:]) * (seg[b] != 0)
        count[b] = values.size - first
        index.append(values[first:] - 1)
        size.append(n[first:])
        cls.append(lab[values[first:] - 1])
    return (ids, count, np.concatenate(cls).astype(np.uint8), np.concatenate(size).astype(np.int32),
            np.concatenate(index).astype(np.int32))


def filter_ref(labels, things, min_voxels, connectivity=26):
    """A copy of labels in which every voxel of a things component of fewer than min_voxels voxels is 0."""
    labels = _np(labels)
    seg = segments_ref(labels, things, (), connectivity).astype(np.int64)
    out = labels.copy()
    for b in range(labels.shape[0]):
        size = np.bincount(seg[b].reshape(-1))
        small = (seg[b] != 0) & (size[seg[b]] < int(min_voxels))
        out[b][small] = 0
    return out


def valid_ref(target, mask=None):
    valid = _np(target) != 255
    if mask is not None:
        valid = valid & _np(mask).reshape(valid.shape).astype(bool)
    return valid


def overlaps_ref(g_ids, g_count, p_ids, p_count, target, mask=None):
    """-> rows (R, 3) int32 (g, p, n): the GLOBAL ids (the exclusive scan of count over the frames + id; 0 = no segment) of
    every pair, not both 0, that a valid voxel carries, ascending in (g, p), and the number of those voxels."""
    g_ids, p_ids = _np(g_ids).astype(np.int64), _np(p_ids).astype(np.int64)
    B = g_ids.shape[0]
    g_off = np.cumsum(_np(g_count)) - _np(g_count)
    p_off = np.cumsum(_np(p_count)) - _np(p_count)
    valid = valid_ref(target, mask).reshape(g_ids.shape)
    G = np.where(g_ids > 0, g_ids + g_off.reshape((B,) + (1,) * (g_ids.ndim - 1)), 0)
    P = np.where(p_ids > 0, p_ids + p_off.reshape((B,) + (1,) * (p_ids.ndim - 1)), 0)
    sel = valid & ((G | P) != 0)
    if not sel.any():
        return np.zeros((0, 3), dtype=np.int32)
    pairs, n = np.unique(np.stack([G[sel], P[sel]], 1), axis=0, return_counts=True)
    return np.concatenate([pairs, n[:, None]], 1).astype(np.int32)


def panoptic_ref(pred_labels, target, n_classes, things, stuff, connectivity=26, min_pred_voxels=1, mask=None,
                 target_instances=None):
    """The counters of PanopticMetrics after one add_batch, segment by segment in plain loops -> (counts (6, C) int64 with
    the rows TP, FP, FN, N_PRED, N_GT, N_DAGGER; sums (2, C) float64: the IoU of the matches added in (frame, g) order, and
    the IoU of every (frame, stuff class) unit)."""
    pred, target = _np(pred_labels).astype(np.uint8), _np(target).astype(np.uint8)
    C = int(n_classes)
    if int(min_pred_voxels) > 1:
        pred = filter_ref(pred, things, min_pred_voxels, connectivity)
    seg_p = segments_ref(pred, things, stuff, connectivity)
    seg_g = (segments_ref(target, things, stuff, connectivity) if target_instances is None
             else instance_segments_ref(target, target_instances, things, stuff))
    valid = valid_ref(target, mask)
    counts, sums = np.zeros((6, C), dtype=np.int64), np.zeros((2, C), dtype=np.float64)
    stuff = set(int(c) for c in stuff)
    for b in range(pred.shape[0]):
        v = valid[b].reshape(-1)
        sg, sp = seg_g[b].reshape(-1)[v].astype(np.int64), seg_p[b].reshape(-1)[v].astype(np.int64)
        lg, lp = target[b].reshape(-1), pred[b].reshape(-1)
        size_g, size_p = np.bincount(sg), np.bincount(sp)
        gs = [g for g in np.flatnonzero(size_g) if g]
        ps = [p for p in np.flatnonzero(size_p) if p]
        for g in gs:
            counts[N_GT, lg[g - 1]] += 1
        for p in ps:
            counts[N_PRED, lp[p - 1]] += 1
        units = set((int(lg[g - 1]),) for g in gs if int(lg[g - 1]) in stuff) | set((int(lp[p - 1]),) for p in ps if int(lp[p - 1]) in stuff)
        for (c,) in units:
            counts[N_DAGGER, c] += 1
        both = (sg > 0) & (sp > 0)
        pairs, n = np.unique(np.stack([sg[both], sp[both]], 1), axis=0, return_counts=True)     # ascending in (g, p)
        for (g, p), inter in zip(pairs.tolist(), n.tolist()):
            c = int(lg[g - 1])
            if int(lp[p - 1]) != c:
                continue
            union = int(size_g[g]) + int(size_p[p]) - inter
            if c in stuff:
                sums[1, c] += inter / union
            if 2 * inter > union:
                counts[TP, c] += 1
                sums[0, c] += inter / union
    counts[FN] = counts[N_GT] - counts[TP]
    counts[FP] = counts[N_PRED] - counts[TP]
    return counts, sums


def panoptic_stats(counts, sums, things, stuff):
    """counts (6, C) int64, sums (2, C) float64 -> the statistics `PanopticMetrics.get_stats` returns."""
    counts, sums = np.asarray(counts, dtype=np.int64), np.asarray(sums, dtype=np.float64)
    C = counts.shape[1]
    tp, fp, fn = (counts[i].astype(np.float64) for i in (TP, FP, FN))
    denom = tp + 0.5 * fp + 0.5 * fn
    present = denom > 0
    pq = np.divide(sums[0], denom, out=np.zeros(C), where=present)
    sq = np.divide(sums[0], tp, out=np.zeros(C), where=tp > 0)
    rq = np.divide(tp, denom, out=np.zeros(C), where=present)
    is_thing, is_stuff = np.zeros(C, dtype=bool), np.zeros(C, dtype=bool)
    is_thing[[c for c in things if c < C]] = True
    is_stuff[[c for c in stuff if c < C]] = True
    dagger = np.where(is_stuff, np.divide(sums[1], counts[N_DAGGER], out=np.zeros(C), where=counts[N_DAGGER] > 0), pq)

    def mean(x, sel):
        sel = sel & present
        return float(x[sel].mean()) if sel.any() else 0.0

    both = is_thing | is_stuff
    return {"PQ_class": pq, "SQ_class": sq, "RQ_class": rq, "PQ_dagger_class": dagger, "present": present & both,
            "PQ": mean(pq, both), "SQ": mean(sq, both), "RQ": mean(rq, both), "PQ_things": mean(pq, is_thing),
            "PQ_stuff": mean(pq, is_stuff), "PQ_dagger": mean(dagger, both),
            "TP": counts[TP].copy(), "FP": counts[FP].copy(), "FN": counts[FN].copy(),
            "pred_segments": counts[N_PRED].copy(), "target_segments": counts[N_GT].copy()}


# ----------------------------------------------------------------------------------------------------- the metric
def _u8_labels(t, name):
    if not torch.is_tensor(t) or t.dim() != 4 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError("%s must be a (B, X, Y, Z) integer label tensor, got %s %s"
                         % (name, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, getattr(t, "dtype", None)))
    return (t if t.dtype == torch.uint8 else t.to(torch.uint8)).contiguous()


class PanopticMetrics:
    """PQ / SQ / RQ of label volumes.  The components, their numbering, the overlap counts and their sort run on the GPU
    (hip.ccl_segments, hip.ccl_compact, hip.ccl_overlaps); the rows -- one per overlapping pair of segments -- and the
    segment tables come to the host, where the matching is a few integer comparisons.  add_batch synchronises with the
    host (the segment counts size the tables)."""

    def __init__(self, n_classes, things, stuff, connectivity=26, min_pred_voxels=1):
        self.n_classes = int(n_classes)
        self.things = tuple(sorted(set(int(c) for c in things)))
        self.stuff = tuple(sorted(set(int(c) for c in stuff)))
        if not 1 <= self.n_classes <= 255:
            raise ValueError("n_classes must be 1..255, got %r" % (n_classes,))
        if set(self.things) & set(self.stuff):
            raise ValueError("things %r and stuff %r overlap" % (self.things, self.stuff))
        if any(not 0 <= c < self.n_classes for c in self.things + self.stuff):
            raise ValueError("things / stuff classes must be 0..%d" % (self.n_classes - 1))
        if int(connectivity) not in (6, 26):
            raise ValueError("connectivity must be 6 or 26, got %r" % (connectivity,))
        if int(min_pred_voxels) < 1:
            raise ValueError("min_pred_voxels must be >= 1, got %r" % (min_pred_voxels,))
        self.connectivity, self.min_pred_voxels = int(connectivity), int(min_pred_voxels)
        self._counts = np.zeros((6, self.n_classes), dtype=np.int64)
        self._sums = np.zeros((2, self.n_classes), dtype=np.float64)
        self._workspace = None

    def _ws(self, labels):
        ws = self._workspace
        if ws is None or ws[0].numel() < labels.numel() or ws[1].numel() < 256 * labels.shape[0] or ws[0].device != labels.device:
            ws = self._workspace = hip.ccl_workspace(labels.shape[0], labels.shape[1:], labels.device)
        return ws

    def _segments(self, labels, instances=None):
        seg = hip.ccl_segments(labels, self.things, self.stuff, self.connectivity, self._ws(labels), instances=instances)
        return hip.ccl_compact(seg, labels)

    def add_batch(self, pred_labels, target, mask=None, target_instances=None):
        """pred_labels, target (B, X, Y, Z) integer labels on the GPU; mask None or bool / uint8 of that size: the voxels
        that count beside target != 255; target_instances None or (B, X, Y, Z) int32 instance ids of the target's things
        voxels (1 .. X Y Z - 1), which then replace the target's components."""
        pred, target = _u8_labels(pred_labels, "pred_labels"), _u8_labels(target, "target").to(pred_labels.device)
        if pred.shape != target.shape:
            raise ValueError("pred_labels %s and target %s differ in shape" % (tuple(pred.shape), tuple(target.shape)))
        if mask is not None:
            if not torch.is_tensor(mask) or mask.numel() != pred.numel() or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("mask must be a bool / uint8 tensor of pred_labels' size %s" % (tuple(pred.shape),))
            mask = mask.reshape(pred.shape).to(pred.device).to(torch.uint8).contiguous()
        if target_instances is not None:
            target_instances = target_instances.reshape(pred.shape).to(pred.device).to(torch.int32).contiguous()
        if self.min_pred_voxels > 1:
            pred = hip.ccl_filter(pred, self.things, self.min_pred_voxels, self.connectivity, self.stuff, self._ws(pred))
        p_ids, p_count, p_off, p_tab = self._segments(pred)
        g_ids, g_count, g_off, g_tab = self._segments(target, target_instances)
        rows = hip.ccl_overlaps(g_ids, g_count, g_off, p_ids, p_count, p_off, target, mask)
        self._match(rows.cpu().numpy(), g_count.numpy(), g_tab[0].cpu().numpy(), p_count.numpy(), p_tab[0].cpu().numpy())
        return self

    def _match(self, rows, g_count, g_class, p_count, p_class):
        """rows (R, 3) of hip.ccl_overlaps, the segment counts per frame and the classes of the segments -> the counters."""
        C = self.n_classes
        rows = rows.astype(np.int64)
        Kg, Kp = int(g_count.sum()), int(p_count.sum())
        g, p, n = rows[:, 0], rows[:, 1], rows[:, 2]
        size_g = np.zeros(Kg + 1, dtype=np.int64)
        size_p = np.zeros(Kp + 1, dtype=np.int64)
        np.add.at(size_g, g, n)
        np.add.at(size_p, p, n)
        cg = np.concatenate([[255], g_class]).astype(np.int64)         # class of a global id; id 0 has none
        cp = np.concatenate([[255], p_class]).astype(np.int64)
        live_g, live_p = size_g > 0, size_p > 0
        live_g[0] = live_p[0] = False
        counts = np.zeros((6, C), dtype=np.int64)
        counts[N_GT] = np.bincount(cg[live_g], minlength=C)[:C]
        counts[N_PRED] = np.bincount(cp[live_p], minlength=C)[:C]
        same = (g > 0) & (p > 0) & (cg[g] == cp[p])
        gs, ps, inter = g[same], p[same], n[same]
        union = size_g[gs] + size_p[ps] - inter
        iou = inter / union
        cls = cg[gs]
        hit = 2 * inter > union
        counts[TP] = np.bincount(cls[hit], minlength=C)[:C]
        counts[FN] = counts[N_GT] - counts[TP]
        counts[FP] = counts[N_PRED] - counts[TP]
        np.add.at(self._sums[0], cls[hit], iou[hit])                   # in row order: (frame, g)
        is_stuff = np.zeros(256, dtype=bool)
        is_stuff[list(self.stuff)] = True
        np.add.at(self._sums[1], cls[is_stuff[cls]], iou[is_stuff[cls]])
        frame_g = np.concatenate([[0], np.repeat(np.arange(len(g_count)), g_count)])
        frame_p = np.concatenate([[0], np.repeat(np.arange(len(p_count)), p_count)])
        sg, sp = live_g & is_stuff[cg], live_p & is_stuff[cp]
        units = np.unique(np.concatenate([frame_g[sg] * 256 + cg[sg], frame_p[sp] * 256 + cp[sp]]))
        counts[N_DAGGER] = np.bincount(units % 256, minlength=C)[:C]
        self._counts += counts

    def reset(self):
        self._counts[:] = 0
        self._sums[:] = 0.0
        return self

    def counts(self):
        """The int64 counters (6, C), rows TP, FP, FN, N_PRED, N_GT, N_DAGGER, as a host tensor."""
        return torch.from_numpy(self._counts.copy())

    def sums(self):
        """The float64 sums (2, C): the IoU of the matches; the IoU of every (frame, stuff class) unit (for PQ_dagger)."""
        return torch.from_numpy(self._sums.copy())

    def merge_(self, other, sums=None):
        """Add the counters of another PanopticMetrics (or its counts() and sums() tensors), e.g. another rank's."""
        if isinstance(other, PanopticMetrics):
            other, sums = other.counts(), other.sums()
        other = torch.as_tensor(other)
        if tuple(other.shape) != self._counts.shape or other.dtype != torch.int64 or sums is None or \
                tuple(torch.as_tensor(sums).shape) != self._sums.shape:
            raise ValueError("merge_ takes (6, %d) int64 counters and (2, %d) float64 sums" % (self.n_classes, self.n_classes))
        self._counts += other.cpu().numpy()
        self._sums += torch.as_tensor(sums).cpu().numpy().astype(np.float64)
        return self

    def allreduce_(self, dist=None):
        """Sum the counters over the ranks of torch.distributed (in place); a no-op without a process group."""
        if dist is None:
            import torch.distributed as dist
            if not dist.is_available():
                return self
        if dist.is_initialized() and dist.get_world_size() > 1:
            dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
            c, s = self.counts().to(dev), self.sums().to(dev)
            dist.all_reduce(c, op=dist.ReduceOp.SUM)
            dist.all_reduce(s, op=dist.ReduceOp.SUM)
            self._counts, self._sums = c.cpu().numpy(), s.cpu().numpy()
        return self

    def get_stats(self):
        """PQ_c = sum of the matches' IoU / (TP + FP / 2 + FN / 2), SQ_c = that sum / TP, RQ_c = TP / (TP + FP / 2 + FN / 2)
        per class (0 where the denominator is 0) -> PQ_class, SQ_class, RQ_class, PQ_dagger_class (C,); PQ, SQ, RQ: their
        means over the things and stuff classes that occur (TP + FP + FN > 0); PQ_things, PQ_stuff; PQ_dagger: as PQ with
        every stuff class scored by its plain IoU (the mean over the frames it occurs in, prediction or target) instead of
        the match at IoU > 1/2; TP, FP, FN, pred_segments, target_segments (C,) int64; present (C,) bool."""
        return panoptic_stats(self._counts, self._sums, self.things, self.stuff)


def format_report(stats, class_names, prefix):
    """The printed block of a PanopticMetrics.get_stats() -> list of lines."""
    lines = ["{}======".format(prefix),
             "PQ={:.4f}, PQ_dagger={:.4f}, SQ={:.4f}, RQ={:.4f}, PQ_things={:.4f}, PQ_stuff={:.4f}".format(
                 stats["PQ"] * 100, stats["PQ_dagger"] * 100, stats["SQ"] * 100, stats["RQ"] * 100, stats["PQ_things"] * 100,
                 stats["PQ_stuff"] * 100),
             "class PQ / SQ / RQ / TP FP FN / segments (prediction, target): {}, ".format(list(class_names))]
    for key in ("PQ_class", "SQ_class", "RQ_class"):
        lines.append(key[:2] + ": " + " ".join("{:.4f}, ".format(v * 100) for v in stats[key].tolist()))
    for key in ("TP", "FP", "FN", "pred_segments", "target_segments"):
        lines.append(key + ": " + " ".join("{:d}, ".format(int(v)) for v in stats[key].tolist()))
    return lines


def remove_small_components(labels, min_voxels, classes=None, connectivity=26):
    """A copy of the GPU label tensor (B, X, Y, Z) or (X, Y, Z), uint8, in which every connected component (6 or 26) of
    fewer than min_voxels voxels of a class in `classes` (None: every class 1..254) is set to 0 (hip.ccl_filter)."""
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() not in (3, 4):
        raise ValueError("labels must be a uint8 (B, X, Y, Z) or (X, Y, Z) tensor")
    classes = tuple(range(1, 255)) if classes is None else tuple(int(c) for c in classes)
    vol = labels.reshape((1,) + tuple(labels.shape)) if labels.dim() == 3 else labels
    return hip.ccl_filter(vol.contiguous(), classes, min_voxels, connectivity).reshape(labels.shape)
