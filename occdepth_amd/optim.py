"""Global gradient-norm clipping fused with the AdamW update (csrc/optim.hip): the "grad-clip 35 -> AdamW" stage of the
reference's training step.  Every configuration the reference ships trains with `gradient_clip_val: 35`
(occdepth/config/*.yaml -> Trainer(gradient_clip_val=...), occdepth/scripts/train.py:188,204), which under Lightning is
`torch.nn.utils.clip_grad_norm_(params, 35)` between the backward and `AdamW.step()`.

    clip_adamw_step(opt, max_norm)        # in place of: clip_grad_norm_(params, max_norm); opt.step()

is a functional step over an ordinary `torch.optim.AdamW`: the state lives in `opt.state[p]` under torch's keys, so
checkpoints, `train_graph._Snapshot`, a resumed reference checkpoint and a later plain `opt.step()` keep working.  On the
GPU it is three launches whatever the number of parameter tensors: per-chunk sums of squares, one workgroup that combines
them in a fixed order into `total_norm` and `clip_coef` (device scalars), and the update, which multiplies the gradient
by `clip_coef` in registers -- `clip_grad_norm_` rewrites every gradient in memory for the same effect.  No atomics and
nothing to zero: deterministic, and capturable into a hipGraph without memset nodes.

The kernels walk a table of 64-byte chunk descriptors (pointers of p, grad, exp_avg, exp_avg_sq, step + offset + count)
that lives in PINNED HOST memory and is read by the device directly, one descriptor per workgroup: nothing is copied, so
a capture records no host-to-device copy that a replay could repeat with stale data.  A table is immutable once a
launch has used it; it is rebuilt (into another buffer) whenever the tuple of data pointers changes -- `torch.cuda.graph`
reallocates the gradients in the graph's pool -- and a table a capture has used is kept for the life of the optimizer.
Pinned memory cannot be allocated while a stream is capturing, so one spare buffer is always kept ready
(`prepare_capture`; `GraphedTrainStep.capture` calls it).

Gradient accumulation (`Trainer(accumulate_grad_batches=N)`, which Lightning skips under manual optimisation):

    w = GradWindow(opt, N)
    w.set(first, last); clip_adamw_step(opt, max_norm, window=w)      # once per micro-batch

adds every micro-batch's gradient, times 1/N, into a float32 accumulator per parameter (one launch); the micro-batch that
closes the window clips the ACCUMULATED gradient by its global norm and applies AdamW to it, the others leave parameters
and optimizer state alone.  Under a capture the position is read from two device ints, so one captured step serves every
position of the window.
"""
import collections
import ctypes
import weakref

import numpy as np
import torch

MAX_EAGER_PLANS = 4           # tables kept for pointer tuples seen outside a capture (least recently used goes first)

_STATES = weakref.WeakKeyDictionary()     # optimizer -> _OptState


def clipping_enabled(max_norm):
    """`gradient_clip_val` semantics of the reference's yaml ("0 FOR w/o gradient clip"): None or 0 = no clipping."""
    return max_norm is not None and float(max_norm) > 0.0


class _Plan:
    """One descriptor table + the device workspace of its launches."""

    def __init__(self, table, n_chunks, n_elems, device, captured):
        self.table = table                                  # pinned (rows >= n_chunks, 8) int64; never rewritten once launched
        self.n_chunks, self.n_elems = n_chunks, n_elems
        self.partials = torch.empty(n_chunks, dtype=torch.float64, device=device)
        self.norm = torch.empty(2, dtype=torch.float32, device=device)      # total_norm, clip_coef
        self.captured = captured                            # a hipGraph may hold launches that read this table: keep it
        self.last_use = None                                # event after the latest eager launch (buffer reuse)


class _OptState:
    def __init__(self):
        self.plans = collections.OrderedDict()              # pointer tuple -> _Plan
        self.spare = None                                   # pinned buffer no launch has used (for a build under capture)
        self.retired = []                                   # (buffer, event) of evicted eager plans


def _state(opt):
    st = _STATES.get(opt)
    if st is None:
        st = _STATES[opt] = _OptState()
    return st


def live_tables(opt, window=None):
    """The objects a captured graph containing `clip_adamw_step(opt, ...)` reads from (descriptor tables, workspaces, and
    with `window` its accumulators, flags and norm): hold the returned list for as long as the graph lives."""
    return list(_state(opt).plans.values()) + ([] if window is None else window.buffers())


def _n_chunks(numel):
    from . import hip
    return max(1, -(-numel // hip.OPTIM_CHUNK))


def _rows_upper_bound(opt):
    return sum(_n_chunks(p.numel()) for g in opt.param_groups for p in g["params"])


def _pinned_rows(rows):
    return torch.empty((max(1, rows), 8), dtype=torch.int64).pin_memory()


def prepare_capture(opt, window=None):
    """Call before `torch.cuda.graph(...)` around a step that uses `clip_adamw_step(opt, ...)`: pinned host memory cannot be
    allocated while a stream is capturing, so the buffer of the table that the capture will build is allocated here.
    With `window`: its device flags, its norm and the accumulator of every parameter that has a gradient or optimizer state
    are allocated too -- an accumulator allocated under the capture would be zeroed again by every replay."""
    st = _state(opt)
    rows = _rows_upper_bound(opt)
    if st.spare is None or st.spare.shape[0] < rows:
        st.spare = _pinned_rows(rows)
    if window is not None:
        for g in opt.param_groups:
            for p in g["params"]:
                if p.is_cuda and p.dtype == torch.float32 and (p.grad is not None or len(opt.state.get(p, ())) != 0):
                    window._device_buffers(p.device)
                    window._accumulator(p, aligned=True)


class GradWindow:
    """A window of `n` micro-batches of one optimizer for `clip_adamw_step(opt, max_norm, window=w)`: owns the float32
    accumulators (one per parameter, created at first use and keyed by the parameter, so they survive the gradient
    re-allocation that builds a new descriptor table; they live OUTSIDE `opt.state`: checkpoints and `state_dict()` do not
    change), the two device ints a captured launch reads its position from, and the device scalars (total_norm, clip_coef)
    of the most recently closed window.

    `set(first, last)` before each step gives the micro-batch's position: `first` overwrites the accumulators (they are
    never zeroed), `last` closes the window.  `is_open` tells whether the latest position left a window open.  A fresh
    window stands at first = last = True: a step without `set` is an ordinary step on scale * g.
    `device_flags`: None = the kernels read the device ints under a stream capture and the host ints otherwise; True /
    False force one of the two (the results are the same bits)."""

    def __init__(self, opt, n, device_flags=None):
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"GradWindow: n must be an int >= 1, got {n!r}")
        self.opt, self.n, self.scale = opt, n, 1.0 / n
        self.device_flags = device_flags
        self.first, self.last, self.is_open = True, True, False
        self.acc = {}                                       # parameter -> accumulator (same shape and strides)
        self.flags = self.norm = self._positions = None     # device buffers, allocated with the first GPU step
        self.last_norm = None                               # torch-sequence path: norm of the last closed window

    def _device_buffers(self, dev):
        if self.flags is None or self.flags.device != dev:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("occdepth_amd.optim: a GradWindow's device buffers cannot be allocated during a stream "
                                   "capture; call optim.prepare_capture(opt, window) before the capture")
            self._positions = torch.tensor([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=torch.int32, device=dev)
            self.flags = self._positions[2 * int(self.first) + int(self.last)].clone()
            self.norm = torch.zeros(2, dtype=torch.float32, device=dev)

    def set(self, first, last):
        """Position of the next micro-batch.  The device ints are filled by a device-to-device copy on the current stream:
        asynchronous, no host synchronisation (compare GraphedTrainStep._sync_decay)."""
        self.first, self.last = bool(first), bool(last)
        self.is_open = not self.last
        if self.flags is not None:
            self.flags.copy_(self._positions[2 * int(self.first) + int(self.last)], non_blocking=True)

    def _accumulator(self, p, aligned):
        """`aligned`: the kernels' layout -- the accumulator shares its parameter's offset to a 16-byte boundary, so the
        128-bit path of the update needs no case of its own."""
        a = self.acc.get(p)
        if a is not None and a.device == p.device and a.shape == p.shape and a.stride() == p.stride() and \
                (not aligned or (a.data_ptr() - p.data_ptr()) % 16 == 0):
            return a
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("occdepth_amd.optim: a gradient accumulator has to be allocated during a stream capture (its "
                               "zero fill would run again in every replay); call optim.prepare_capture(opt, window) first")
        if aligned:
            buf = torch.zeros(p.numel() + 3, dtype=torch.float32, device=p.device)
            k = ((p.data_ptr() - buf.data_ptr()) % 16) // 4
            a = buf[k:k + p.numel()].as_strided(p.shape, p.stride(), k)
            if a.numel() == 0:
                a = torch.zeros_like(p, memory_format=torch.preserve_format)
        else:
            a = torch.zeros_like(p, memory_format=torch.preserve_format)
        self.acc[p] = a
        return a

    def buffers(self):
        return list(self.acc.values()) + [t for t in (self.flags, self.norm, self._positions) if t is not None]

    def state(self):
        """What a step mutates, for `train_graph._Snapshot`: clones of the device buffers + the host position."""
        return ({p: a.detach().clone() for p, a in self.acc.items()},
                None if self.norm is None else self.norm.clone(), (self.first, self.last, self.is_open), self.last_norm)

    def restore(self, saved):
        accs, norm, (first, last, is_open), self.last_norm = saved
        for p, a in self.acc.items():
            if p in accs and accs[p].shape == a.shape:
                a.copy_(accs[p])
            else:
                a.zero_()
        if self.norm is not None:
            if norm is not None:
                self.norm.copy_(norm)
            else:
                self.norm.zero_()
        self.set(first, last)
        self.is_open = is_open


def _fallback(opt, max_norm, out_norm):
    params = [p for g in opt.param_groups for p in g["params"]]
    total = torch.nn.utils.clip_grad_norm_(params, float(max_norm))
    opt.step()
    if out_norm is not None:
        out_norm.copy_(total)
        return out_norm
    return total


def _same_layout(p, *others):
    if not (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)
            or p.is_contiguous(memory_format=torch.channels_last_3d)):
        return False
    return all(t.shape == p.shape and t.stride() == p.stride() for t in others)


def _kernel_operands(opt):
    """(hyper-parameters, [(p, grad, exp_avg, exp_avg_sq, step)]) when the HIP kernels cover this optimizer, else the
    reason (a string) why the torch sequence runs instead.  Creates missing state as torch does for a capturable AdamW."""
    if not isinstance(opt, torch.optim.AdamW):
        return "not a torch.optim.AdamW"
    hyper, lr0 = None, None
    todo = []
    for g in opt.param_groups:
        if g.get("amsgrad") or g.get("maximize") or g.get("differentiable"):
            return "amsgrad / maximize / differentiable"
        h = (tuple(float(b) for b in g["betas"]), float(g["eps"]), float(g["weight_decay"]))
        lr = g["lr"]
        if hyper is None:
            hyper, lr0 = h, lr
        elif h != hyper or not (lr is lr0 or (not torch.is_tensor(lr) and not torch.is_tensor(lr0) and float(lr) == float(lr0))):
            return "param groups with different hyper-parameters"
        for p in g["params"]:
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("AdamW does not support sparse gradients")
            todo.append((g, p))
    if not todo:
        return "no gradients"
    dev = todo[0][1].device
    if dev.type != "cuda":
        return "CPU tensors"
    if torch.is_tensor(lr0) and not (lr0.device == dev and lr0.dtype == torch.float32 and lr0.numel() == 1):
        return "learning-rate tensor off the parameters' device"
    ops = []
    for g, p in todo:
        if p.device != dev or p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.device != dev:
            return "a non-float32 parameter or several devices"
        state = opt.state[p]
        if len(state) == 0:
            if not (g.get("capturable") or g.get("fused")):
                return "host-side step counter (neither capturable nor fused)"
            state["step"] = torch.zeros((), dtype=torch.float32, device=dev)
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step, m, v = state.get("step"), state.get("exp_avg"), state.get("exp_avg_sq")
        if not (torch.is_tensor(step) and step.device == dev and step.dtype == torch.float32 and step.numel() == 1):
            return "host-side step counter"
        if not (torch.is_tensor(m) and torch.is_tensor(v) and m.dtype == v.dtype == torch.float32 and m.device == v.device == dev
                and _same_layout(p, p.grad, m, v)):
            return "optimizer state or gradient laid out unlike its parameter"
        ops.append((p, p.grad, m, v, step))
    return (hyper, lr0), ops


def _build_table(buf, ops):
    """`ops`: (p, grad, exp_avg, exp_avg_sq, step) per tensor, with a window also its accumulator."""
    from . import hip
    chunk = hip.OPTIM_CHUNK
    ptrs = np.array([[t.data_ptr() for t in op] for op in ops], dtype=np.uint64).astype(np.int64)
    numel = np.array([op[0].numel() for op in ops], dtype=np.int64)
    nch = np.maximum(1, -(-numel // chunk))
    idx = np.repeat(np.arange(len(ops)), nch)
    offset = (np.arange(int(nch.sum())) - np.repeat(np.cumsum(nch) - nch, nch)) * chunk
    rows = np.zeros((len(idx), 8), dtype=np.int64)
    rows[:, :5] = ptrs[idx][:, :5]
    if ptrs.shape[1] > 5:
        rows[:, 7] = ptrs[idx][:, 5]                         # occd_optim_chunk.acc
    rows[:, 5] = offset
    rows[:, 6] = np.minimum(chunk, numel[idx] - offset)      # int32 count + int32 zero (little endian)
    assert ctypes.sizeof(hip.OptimChunk) == 64 and rows.shape[0] <= buf.shape[0]
    buf.numpy()[:rows.shape[0]] = rows
    return rows.shape[0], int(numel.sum())


def _plan_for(opt, ops, dev):
    st = _state(opt)
    sig = tuple(x for op in ops for x in tuple(t.data_ptr() for t in op) + (op[0].numel(),))
    capturing = torch.cuda.is_current_stream_capturing()
    plan = st.plans.get(sig)
    if plan is not None:
        st.plans.move_to_end(sig)
        plan.captured = plan.captured or capturing
        return plan, capturing
    rows = sum(_n_chunks(op[0].numel()) for op in ops)
    if capturing:
        if st.spare is None or st.spare.shape[0] < rows:
            raise RuntimeError("occdepth_amd.optim: the descriptor table of this step has to be built during a stream capture "
                               "and no pinned buffer is ready; call optim.prepare_capture(opt) before the capture")
        buf, st.spare = st.spare, None
    else:
        buf = None
        for i, (b, ev) in enumerate(st.retired):
            if b.shape[0] >= rows and ev.query():            # its last launch has finished: nothing reads it any more
                buf = st.retired.pop(i)[0]
                break
        if buf is None:
            buf = _pinned_rows(rows)
    n_chunks, n_elems = _build_table(buf, ops)
    plan = st.plans[sig] = _Plan(buf, n_chunks, n_elems, dev, capturing)
    if not capturing:
        eager = [k for k, pl in st.plans.items() if not pl.captured]
        for k in eager[:max(0, len(eager) - MAX_EAGER_PLANS)]:
            old = st.plans.pop(k)
            if old.last_use is not None:
                st.retired.append((old.table, old.last_use))
        for _, ev in st.retired[:-MAX_EAGER_PLANS]:
            ev.synchronize()                                 # the buffer goes back to the allocator: no launch may still read it
        del st.retired[:-MAX_EAGER_PLANS]
    return plan, capturing


def _window_fallback(opt, max_norm, out_norm, w):
    """torch's own sequence on the window's accumulators: acc = g / n | acc += g / n; closing: p.grad = acc,
    [clip_grad_norm_], opt.step()."""
    params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
    with torch.no_grad():
        for p in params:
            if p.grad.is_sparse:
                raise RuntimeError("AdamW does not support sparse gradients")
            a = w._accumulator(p, aligned=False)
            if w.first:
                torch.div(p.grad, w.n, out=a)
            else:
                a += p.grad / w.n
    clip = clipping_enabled(max_norm)
    if w.last:
        for p in params:
            p.grad = w.acc[p]
        if clip:
            w.last_norm = torch.nn.utils.clip_grad_norm_(params, float(max_norm))
        opt.step()
    if not clip or w.last_norm is None:
        return None
    if out_norm is not None:
        out_norm.copy_(w.last_norm)
        return out_norm
    return w.last_norm


def _window_step(opt, max_norm, out_norm, w):
    if w.opt is not opt:
        raise ValueError("occdepth_amd.optim: this GradWindow belongs to another optimizer")
    got = _kernel_operands(opt)
    if isinstance(got, str):
        return _window_fallback(opt, max_norm, out_norm, w)
    from . import hip
    ((betas, eps, weight_decay), lr), ops = got
    dev = ops[0][0].device
    clip = clipping_enabled(max_norm)
    lib = hip.load()
    with torch.cuda.device(dev):
        w._device_buffers(dev)
        ops = [op + (w._accumulator(op[0], aligned=True),) for op in ops]
        plan, capturing = _plan_for(opt, ops, dev)
        a = hip.AccumAdamWArgs()
        a.chunks, a.partials, a.norm_out = plan.table.data_ptr(), plan.partials.data_ptr(), w.norm.data_ptr()
        a.n_chunks, a.n_elems = plan.n_chunks, plan.n_elems
        if torch.is_tensor(lr):
            a.lr_dev, a.lr = lr.data_ptr(), 0.0
        else:
            a.lr_dev, a.lr = None, float(lr)
        a.beta1, a.beta2, a.eps, a.weight_decay = betas[0], betas[1], eps, weight_decay
        a.max_norm, a.scale = (float(max_norm) if clip else 0.0), w.scale
        on_device = capturing if w.device_flags is None else bool(w.device_flags)
        if capturing and not on_device:
            raise RuntimeError("occdepth_amd.optim: a captured step reads the window position from the device flags")
        a.flags_dev = w.flags.data_ptr() if on_device else None
        a.first, a.last = int(w.first), int(w.last)
        hip._check(lib.occd_accum_clip_adamw(ctypes.byref(a), hip._stream()), "occd_accum_clip_adamw")
        if not capturing:
            if plan.last_use is None:
                plan.last_use = torch.cuda.Event()
            plan.last_use.record()
            st = _state(opt)
            if st.spare is None:                             # the next build may happen under a capture
                st.spare = _pinned_rows(_rows_upper_bound(opt))
    if not clip:
        return None
    total = w.norm[0]
    if out_norm is not None:
        out_norm.copy_(total)
        return out_norm
    return total


def clip_adamw_step(opt, max_norm, *, out_norm=None, window=None):
    """`torch.nn.utils.clip_grad_norm_(params, max_norm)` followed by `opt.step()` for a `torch.optim.AdamW`, returning the
    total norm (a 0-dim tensor; also copied into `out_norm` when given).

    `p.grad` is left UNSCALED on the kernel path: the clip coefficient is applied in registers inside the update, the
    gradients in memory are what the backward (and the gradient average) wrote.  The parameters, `exp_avg`, `exp_avg_sq` and
    `step` afterwards are those of the torch sequence.  Parameters whose `.grad` is None are skipped and their `step` is not
    advanced; sparse gradients raise.  `max_norm` None or 0: no clipping, plain `opt.step()`, returns None.

    The HIP kernels run when every parameter with a gradient is a float32 CUDA tensor of one device and the optimizer is a
    plain AdamW (no amsgrad / maximize) with device-side step counters (`capturable`, see train_graph.make_capturable) and
    one set of hyper-parameters; a learning rate held in a device tensor is read by the kernel, so a scheduler's change
    reaches a captured launch.  Anything else -- CPU tensors among them -- runs the torch sequence itself, with the same
    result.  The choice depends on these properties only: with the model on the GPU and libocc_hip.so missing this raises.

    `window` (a `GradWindow` of this optimizer, position given by `window.set(first, last)`): gradient accumulation.  The
    gradient, times 1/n, is added into the window's accumulators (written, not added, when `first`); only when `last` are
    the accumulated gradients clipped by THEIR global norm and applied -- otherwise parameters, moments, `step` and the norm
    keep their bits.  `step` counts windows.  Returns the norm of the most recently closed window (a 0-dim device scalar
    that later steps and replays keep up to date), or None when clipping is off, which with a window still accumulates.
    The same conditions choose between the kernels (`p.grad` is never written) and the torch sequence on the same
    accumulators, where -- on this path only -- the closing step REPLACES `p.grad` by the accumulator, which
    `clip_grad_norm_` then scales in place.  Every micro-batch of a window must bring gradients for the same parameters."""
    if window is not None:
        return _window_step(opt, max_norm, out_norm, window)
    if not clipping_enabled(max_norm):
        opt.step()
        return None
    got = _kernel_operands(opt)
    if isinstance(got, str):
        return _fallback(opt, max_norm, out_norm)
    from . import hip
    ((betas, eps, weight_decay), lr), ops = got
    dev = ops[0][0].device
    lib = hip.load()
    with torch.cuda.device(dev):
        plan, capturing = _plan_for(opt, ops, dev)
        a = hip.ClipAdamWArgs()
        a.chunks, a.partials, a.norm_out = plan.table.data_ptr(), plan.partials.data_ptr(), plan.norm.data_ptr()
        a.n_chunks, a.n_elems = plan.n_chunks, plan.n_elems
        if torch.is_tensor(lr):
            a.lr_dev, a.lr = lr.data_ptr(), 0.0
        else:
            a.lr_dev, a.lr = None, float(lr)
        a.beta1, a.beta2, a.eps, a.weight_decay, a.max_norm = betas[0], betas[1], eps, weight_decay, float(max_norm)
        hip._check(lib.occd_clip_adamw(ctypes.byref(a), hip._stream()), "occd_clip_adamw")
        if not capturing:
            if plan.last_use is None:
                plan.last_use = torch.cuda.Event()
            plan.last_use.record()
            st = _state(opt)
            if st.spare is None:                             # the next build may happen under a capture
                st.spare = _pinned_rows(_rows_upper_bound(opt))
    total = plan.norm[0]
    if out_norm is not None:
        out_norm.copy_(total)
        return out_norm
    return total


def grad_norm(opt, max_norm=1.0):
    """`total_norm` of the optimizer's gradients by the norm pass alone (no update, `step` untouched): what
    `clip_adamw_step` would measure.  GPU kernel path only."""
    got = _kernel_operands(opt)
    if isinstance(got, str):
        raise RuntimeError(f"occdepth_amd.optim.grad_norm: the HIP kernels do not cover this optimizer ({got})")
    from . import hip
    _, ops = got
    dev = ops[0][0].device
    with torch.cuda.device(dev):
        plan, capturing = _plan_for(opt, ops, dev)
        a = hip.ClipAdamWArgs()
        a.chunks, a.partials, a.norm_out = plan.table.data_ptr(), plan.partials.data_ptr(), plan.norm.data_ptr()
        a.n_chunks, a.n_elems, a.max_norm = plan.n_chunks, plan.n_elems, float(max_norm)
        hip._check(hip.load().occd_grad_sumsq(ctypes.byref(a), hip._stream()), "occd_grad_sumsq")
        if not capturing:
            if plan.last_use is None:
                plan.last_use = torch.cuda.Event()
            plan.last_use.record()
    return plan.norm[0].clone()
