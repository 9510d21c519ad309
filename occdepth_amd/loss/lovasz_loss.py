"""Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018): the convex surrogate of the per-class Jaccard index, the term
that optimises what mIoU measures.  Over the whole batch (per_image=False) and the classes present in the target.

    loss = LovaszSoftmaxLoss()(ssc_logit, target)             # logits (B, C, X, Y, Z), target (B, X, Y, Z) uint8, 255 = unknown

For class c and valid voxel i: fg = [y_i == c], p = softmax(z_i)[c], e = fg ? 1 - p : p.  The valid voxels are ordered by
descending e (ties: ascending voxel index); with J_k the Jaccard loss 1 - |fg n top_k| / |fg u top_k| of the first k of
them, g_k = J_k - J_{k-1},  L_c = sum_k e_(k) g_k,  L = mean of L_c over the classes with a foreground voxel; g is a constant
of the gradient.  The specification is in include/occdepth_amd.h; GPU float32 logits run on csrc/sort.hip (K38, the stable
segmented radix sort) and csrc/lovasz.hip (`hip.lovasz_*`; a missing library is an error), everything else -- CPU tensors,
other dtypes -- on the torch formulation below.
"""
import numpy as np
import torch

from .. import hip


# ------------------------------------------------------------------------------------------- the torch formulation
def _flatten(logits, target):
    if logits.dim() < 3:
        raise ValueError("logits must be (B, C, ...), got %s" % (tuple(logits.shape),))
    if tuple(target.shape) != (logits.shape[0],) + tuple(logits.shape[2:]):
        raise ValueError("target %s does not match logits %s" % (tuple(target.shape), tuple(logits.shape)))
    C = logits.shape[1]
    hip.lovasz_check_voxels(target.numel())
    return logits.reshape(logits.shape[0], C, -1).permute(0, 2, 1).reshape(-1, C), target.reshape(-1)


def lovasz_softmax_torch(logits, target, ignore=255):
    """The published formulation (lovasz_softmax_flat with classes='present', per_image=False) with a stable sort;
    differentiable in logits, any float dtype, any device."""
    z, y = _flatten(logits, target)
    keep = y != ignore
    prob = torch.softmax(z, 1)[keep]
    y = y[keep]
    losses = []
    for c in range(prob.shape[1]):
        fg = (y == c).to(prob.dtype)
        if fg.sum() == 0:
            continue
        err = (fg - prob[:, c]).abs()
        err_sorted, perm = torch.sort(err, dim=0, descending=True, stable=True)
        fg_sorted = fg[perm]
        total = fg_sorted.sum()
        inter = total - fg_sorted.cumsum(0)
        union = total + (1.0 - fg_sorted).cumsum(0)
        jac = 1.0 - inter / union
        grad = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(err_sorted, grad.detach()))
    if not losses:
        return z.sum() * 0.0
    return torch.stack(losses).mean()


# ------------------------------------------------------------------------------------------ the float64 restatement
def lovasz_ref_from_errors(err, fg, valid):
    """Straight from the definition, on ready-made errors: err (C, N), fg (C, N) bool, valid (N,) bool ->
    (L_c (C,) float64, 0 for an absent class; g (C, N) float64: d L_c / d err, 0 at invalid voxels).  The Jaccard losses
    of the prefixes come from cumulative sums and g from their differences, in numpy's widest float (the differences
    cancel: J_k - J_{k-1} carries an absolute error of one unit of J)."""
    wide = np.longdouble
    err, fg, valid = np.asarray(err, np.float64), np.asarray(fg, bool), np.asarray(valid, bool)
    C, N = err.shape
    Lc, g = np.zeros(C, np.float64), np.zeros((C, N), np.float64)
    idx = np.flatnonzero(valid)
    for c in range(C):
        f = fg[c, idx]
        if not f.any():
            continue
        e = err[c, idx]
        order = np.argsort(-e, kind="stable")
        fs = f[order].astype(wide)
        total = fs.sum()
        inter = total - np.cumsum(fs)
        union = total + np.cumsum(1 - fs)
        jac = 1 - inter / union
        d = np.diff(jac, prepend=wide(0))
        Lc[c] = float(np.sum(e[order].astype(wide) * d))
        g[c, idx[order]] = d.astype(np.float64)
    return Lc, g


def lovasz_ref(logits, target, ignore=255):
    """float64 numpy restatement from the cumsum / Jaccard definition: logits (B, C, ...), target (B, ...) ->
    (loss, per-class losses (C,), gradient of the loss in the logits, of their shape)."""
    z = np.asarray(logits, np.float64)
    y = np.asarray(target).reshape(-1)
    B, C = z.shape[:2]
    rows = np.moveaxis(z.reshape(B, C, -1), 1, 2).reshape(-1, C)
    p = np.exp(rows - rows.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    fg = y[None, :] == np.arange(C)[:, None]
    valid = y != ignore
    err = np.where(fg, 1.0 - p.T, p.T)
    Lc, g = lovasz_ref_from_errors(err, fg & valid[None], valid)
    present = max(1, int((fg & valid[None]).any(1).sum()))
    loss = Lc.sum() / present
    dp = (np.where(fg, -g, g) / present).T                                  # (N, C): d L / d p
    dz = p * (dp - (dp * p).sum(1, keepdims=True))
    return loss, Lc, np.moveaxis(dz.reshape(B, -1, C), 2, 1).reshape(z.shape)


# ----------------------------------------------------------------------------------------------------- the HIP path
class _LovaszSoftmax(torch.autograd.Function):
    """Errors pass, K38 sort, ranks pass; backward voxel pass (csrc/lovasz.hip).  The `_DepthBCE` / `_RenderDepth` pattern:
    #present and the incoming gradient stay on the device (gscale), no host read, capture-safe."""

    @staticmethod
    def forward(ctx, logits, target, class_chunk, ignore):
        q, fg_count, loss_q = hip.lovasz_forward(logits, target, class_chunk, ignore)
        present = (fg_count > 0).sum().clamp(min=1).double()
        ctx.save_for_backward(logits, target, q, present)
        ctx.ignore = ignore
        ctx.mark_non_differentiable(fg_count, loss_q)
        return (loss_q.double().sum() / (float(1 << hip.LOVASZ_Q) * present)).float(), fg_count, loss_q

    @staticmethod
    def backward(ctx, g, *unused):
        logits, target, q, present = ctx.saved_tensors
        gscale = (g.double() / present).float().reshape(1)
        return hip.lovasz_bwd(logits, target, q, gscale, ctx.ignore), None, None, None


class LovaszSoftmaxLoss:
    """loss = LovaszSoftmaxLoss(class_chunk)(logits, target): logits (B, C, ...), target (B, ...) uint8, `ignore` unknown.
    class_chunk: classes sorted at a time over the same scratch (default: all; `hip.lovasz_scratch_bytes`).  After a call on
    the kernels, `last` holds (G_c, L_c in Q60) of that call, both (C,) int64."""

    def __init__(self, class_chunk=None, ignore=255):
        if class_chunk is not None and int(class_chunk) < 1:
            raise ValueError("class_chunk must be >= 1, got %r" % (class_chunk,))
        self.class_chunk = None if class_chunk is None else int(class_chunk)
        self.ignore = int(ignore)
        self.last = None

    def __call__(self, logits, target):
        _flatten(logits, target)                                             # shape and N < 2^31 checks
        target = target.to(logits.device)
        if hip.lovasz_usable(logits):
            if target.dtype != torch.uint8:
                target = target.to(torch.uint8)
            chunk = None if self.class_chunk is None else min(self.class_chunk, int(logits.shape[1]))
            loss, fg_count, loss_q = _LovaszSoftmax.apply(logits, target, chunk, self.ignore)
            self.last = (fg_count, loss_q)
            return loss
        self.last = None
        return lovasz_softmax_torch(logits, target, self.ignore)
