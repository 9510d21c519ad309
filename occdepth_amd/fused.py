"""Eval-mode execution plans: nn.Conv3d / ConvTranspose3d / AvgPool3d+Conv3d (+ BatchNorm3d)
folded into one packed-weight launch of the HIP implicit-GEMM kernel (K2).

A plan owns no parameters: it references the live nn modules and folds BatchNorm running
statistics into (weight scale, bias) on first use; the folded weights (a PackedW) are rebuilt
whenever a source tensor is replaced or modified in place (load_state_dict, optimizer step),
detected through (data_ptr, _version).  Which kernel a launch takes is decided per launch by
route(); a weight image is packed at the first launch that routes to it.
"""
import os

import torch

from . import hip
from .hip import ACT_NONE, ACT_RELU, ACT_RELU_PRE, ACT_SIGMOID, Vox  # noqa: F401 (re-exported)


_warned_eval_with_grad = False


def needs_autograd(module):
    """True when the differentiable ATen graph must be built (training, or eval with gradients enabled);
    the HIP eval path is forward-only and is taken under torch.no_grad() / torch.inference_mode()."""
    if module.training:
        return True
    if torch.is_grad_enabled():
        global _warned_eval_with_grad
        if not _warned_eval_with_grad:
            _warned_eval_with_grad = True
            import warnings
            warnings.warn("occdepth_amd: eval-mode forward with autograd enabled runs the differentiable ATen path; "
                          "wrap inference in torch.no_grad() to take the HIP eval path", stacklevel=3)
        return True
    return False


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (int(v),) * 3


def on_gpu(t):
    """Gate of the 2-D eval fast paths (fused HIP kernels instead of ATen).  A function, not `t.is_cuda` inline, so that the
    CPU test-suite can drive the very same host logic through its torch emulation of the kernels (tests/emu.py)."""
    return t.is_cuda


def _stamp(*mods):
    key = []
    for m in mods:
        if m is None:
            continue
        for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
            key.append((t.data_ptr(), t._version, t.device))
    return tuple(key)


def _bn_affine(bn, cout, device):
    """BatchNorm (eval) as y = x * scale + shift."""
    if bn is None:
        return None, torch.zeros(cout, device=device)
    inv = torch.rsqrt(bn.running_var.float() + bn.eps)
    g = bn.weight.float() if bn.weight is not None else torch.ones_like(inv)
    b = bn.bias.float() if bn.bias is not None else torch.zeros_like(inv)
    scale = g * inv
    return scale, b - bn.running_mean.float() * scale


def bn_affine_cached(bn):
    """(scale, shift) of an eval-mode BatchNorm, cached on the module until its tensors change."""
    key = _stamp(bn)
    cached = getattr(bn, "_occd_affine", None)
    if cached is None or cached[0] != key:
        scale, shift = _bn_affine(bn, bn.num_features, bn.running_mean.device)
        cached = (key, scale.contiguous(), shift.contiguous())
        bn._occd_affine = cached
    return cached[1], cached[2]


def _same(*values):
    return {v: v for v in values}


# The switches that take a value out of a set, declared once: name -> (environment variable, value when it is unset, value
# when it is empty, {accepted spelling: value}, the "expected ..." text of the error).
_SWITCHES = {
    # Which kernel the fused Winograd 3x3 convolutions of the eval forward take (the decoder levels of unet2d.py, DepthNet's 3x3 +
    # BatchNorm + ReLU of flosp_depth.py):
    #   OCCDEPTH_WINO_SPLIT=f16x2  (default) K10h, K10 on the f16 matrix pipe with the two-term fp16 split, wherever
    #                              hip.wino_f16x2_wins says it is faster (per launch geometry); error against float64 within 2x of
    #                              K10's (tests/test_wino_f16x2.py); finite activations |x| >= 8190 overflow to non-finite outputs
    #                              (INTEGRATION.md section 6); weights that are not all finite keep K10
    #   OCCDEPTH_WINO_SPLIT=fp32   K10 everywhere (the bit-for-bit previous path)
    # Training (hip.conv2d_3x3_autograd) is K10 in either mode.
    "WINO_SPLIT": ("OCCDEPTH_WINO_SPLIT", "f16x2", "f16x2", _same("f16x2", "fp32"), "f16x2 or fp32"),
    # The 3-way bf16 split (x = hi + mid + lo, six bf16 MFMAs per K step, float32-level accuracy on the bf16 matrix pipe):
    #   OCCDEPTH_BF16X3=head  (default since round 4) the full-resolution head convolutions (<= 32 -> <= 32 channels, 3x3x3,
    #                         dilation 1 / 2 / 3, Z = 32) on K2s3, the sliding-window form of the split (csrc/conv3d_c32p.hip;
    #                         since ABI 15 by default on its fp16 two-term twin K2s3h instead, see OCCDEPTH_HEAD_SPLIT below):
    #                         0.51 ms per launch against 0.90 ms for the exact-fp32 K2s, error against float64 no larger than
    #                         K2s' own (tests/test_bf16_conv.py::test_conv3d_slide_x3_head_kernel, profiles/r04_head_x3_ab.txt);
    #                         also (see below) the long-K 3x3x3 convolutions of small volumes and the merged phase launches of the
    #                         transposed convolutions on K2b's split form; everything else exact fp32
    #   OCCDEPTH_BF16X3=0     exact-fp32 MFMA everywhere (v_mfma_f32_32x32x2_f32): the bit-for-bit round-3 path
    #   OCCDEPTH_BF16X3=1     additionally every other large dilation-1 K2 launch on the generic K2b skeleton with the split
    #                         (csrc/conv3d_bf16.hip; the round-3 experiment)
    "BF16X3": ("OCCDEPTH_BF16X3", "head", "0", {"0": False, "": False, "off": False, "false": False, "1": "all", "all": "all",
                                                "on": "all", "true": "all", "head": "head"}, "0, head or 1"),
    # Which split the full-resolution head launches (K2s3's geometry) take while the split is on (OCCDEPTH_BF16X3 != 0):
    #   OCCDEPTH_HEAD_SPLIT=f16x2   (default) K2s3h, the two-term fp16 split: x = hi + 2^-11 lo', three v_mfma_f32_32x32x16_f16
    #                               per K step instead of six bf16 ones; error against float64 within 2x of the exact-fp32 K2s
    #                               (tests/test_head_f16x2.py); finite activations |x| >= 32760 overflow to non-finite outputs
    #                               (INTEGRATION.md section 6); plans whose weights are not all finite keep bf16x3
    #   OCCDEPTH_HEAD_SPLIT=bf16x3  K2s3 as before (the bit-for-bit previous path)
    # Everything else -- the K2b split launches, the 2-D GEMMs, training (autograd3d.py) -- is unchanged by this switch.
    "HEAD_SPLIT": ("OCCDEPTH_HEAD_SPLIT", "f16x2", "f16x2", _same("f16x2", "bf16x3"), "f16x2 or bf16x3"),
    # Which split K2b's float32-accurate launches take while the split is on (OCCDEPTH_BF16X3 != 0) -- the long-K 3x3x3
    # convolutions of small volumes and the merged phase launches of the transposed convolutions:
    #   OCCDEPTH_K2B_SPLIT=f16x2   (default) K2bh, K2s3h's numerics on the generic kernel (csrc/conv3d_bf16.hip, SPLIT = 2): three
    #                              v_mfma_f32_32x32x16_f16 per K step and 4 streamed bytes per weight element instead of six MFMAs
    #                              and 6 bytes; error against float64 within 2x of the exact-fp32 K2 (tests/test_k2b_f16x2.py);
    #                              finite activations |x| >= 32760 overflow to non-finite outputs;
    #                              plans whose weights are not all finite keep bf16x3
    #   OCCDEPTH_K2B_SPLIT=bf16x3  the three-term bf16 split as before (the bit-for-bit previous path)
    # The head launches (OCCDEPTH_HEAD_SPLIT), the OCCDEPTH_BF16X3=1 experiment, the opt-in 1x1x1 / sigmoid route and training
    # are unchanged by this switch.
    "K2B_SPLIT": ("OCCDEPTH_K2B_SPLIT", "f16x2", "f16x2", _same("f16x2", "bf16x3"), "f16x2 or bf16x3"),
    # Which weight image the 2-D network's operand holders (hip.GemmWeights of efficientnet.gemm_operands, the tap-GEMM and the
    # merged conv_head o conv2 operands of unet2d.py) make for the GEMMs that read pre-split weights -- K16p, K21 and K16's
    # pre-split form (csrc/gemm_x3.hip):
    #   OCCDEPTH_GEMM_SPLIT=f16x2   (default) the image of occd_gemm_f16x2_pack: three v_mfma_f32_32x32x16_f16 per K step and 4
    #                               streamed bytes per weight element instead of six bf16 MFMAs and 6 bytes; error against float64
    #                               within the bounds of tests/test_gemm_f16x2.py; finite activations |x| >= 32760 overflow to
    #                               non-finite outputs; matrices with a non-finite weight keep bf16x3
    #   OCCDEPTH_GEMM_SPLIT=bf16x3  the three-term bf16 image as before (the bit-for-bit previous path)
    # Under f16x2 the builders also put the Winograd-domain products of the decoder on the channel-major form (hip.WinoCM, where
    # hip.wino_cm_wins says so) and the K16 launches below 256 rows (project convolutions with gate and residual, the 192-row
    # expand) on the image (hip.tile_f16x2_wins); bf16x3 keeps their float32 operands, bit for bit as before.
    # Explicit hip.GemmPacked(w, role) / hip.GemmWeights(w, role) callers, role-"b" images and training are unchanged by this
    # switch.
    "GEMM_SPLIT": ("OCCDEPTH_GEMM_SPLIT", "f16x2", "f16x2", _same("f16x2", "bf16x3"), "f16x2 or bf16x3"),
}


def _parse(name, v):
    env, _, empty, spellings, expected = _SWITCHES[name]
    v = (v or empty).strip().lower()
    if v not in spellings:
        raise ValueError(f"{env}={v!r}: expected {expected}")
    return spellings[v]


def _from_env(name):
    return _parse(name, os.environ.get(*_SWITCHES[name][:2]))


WINO_SPLIT, BF16X3 = _from_env("WINO_SPLIT"), _from_env("BF16X3")
HEAD_SPLIT, K2B_SPLIT = _from_env("HEAD_SPLIT"), _from_env("K2B_SPLIT")
GEMM_SPLIT = _from_env("GEMM_SPLIT")


def set_wino_split(v):
    """'f16x2' / 'fp32'; the cached operands are re-packed on the next call."""
    global WINO_SPLIT
    WINO_SPLIT = _parse("WINO_SPLIT", v)


def set_bf16x3(on):
    """False / 'head' / 'all' (True = 'all'); takes effect at the next launch."""
    global BF16X3
    BF16X3 = "all" if on is True else _parse("BF16X3", str(on)) if on else False


def set_head_split(v):
    """'f16x2' / 'bf16x3'; takes effect at the next launch."""
    global HEAD_SPLIT
    HEAD_SPLIT = _parse("HEAD_SPLIT", v)


def set_k2b_split(v):
    """'f16x2' / 'bf16x3'; takes effect at the next launch."""
    global K2B_SPLIT
    K2B_SPLIT = _parse("K2B_SPLIT", v)


def set_gemm_split(v):
    """'f16x2' / 'bf16x3'; the operand builders re-pack on the next call (hip.set_gemm_split is the same switch)."""
    global GEMM_SPLIT
    GEMM_SPLIT = _parse("GEMM_SPLIT", v)


def wino_pack(w, scale=None):
    """The weight operand of hip.conv2d_3x3_fused under the current WINO_SPLIT: K10's float32 image, or (f16x2, GPU tensors,
    finite weights) K10h's image with K10's beside it for the launch geometries that stay on K10."""
    f32 = hip.wino_pack_weights(w, scale)
    if WINO_SPLIT != "f16x2" or not w.is_cuda:             # (CPU tensors: the emulated path of the host-logic tests)
        return f32
    try:
        upk = hip.wino_pack_weights_f16x2(w, scale)
    except ValueError:                                     # non-finite weights: no power-of-two scale
        return f32
    upk.f32 = f32
    return upk


def wino_fused_operands(owner, conv, bn):
    """(packed Winograd-domain weights of K10 / K10h with the BatchNorm scale folded in, shift) of a 3x3 convolution +
    BatchNorm, cached on `owner` until a source tensor changes ((data_ptr, _version) stamp) or the split is switched."""
    key = (_stamp(conv, bn), WINO_SPLIT)
    cache = owner.__dict__.setdefault("_fused_cache", {})
    hit = cache.get(id(conv))
    if hit is None or hit[0] != key:
        scale, shift = bn_affine_cached(bn)
        if conv.bias is not None:
            shift = shift + scale * conv.bias.detach().float()
        hit = (key, wino_pack(conv.weight, scale), shift.contiguous())
        cache[id(conv)] = hit
    return hit[1:]


def _pad_bias(bias, cout):
    out = torch.zeros(hip.round_up(cout, 32), device=bias.device, dtype=torch.float32)
    out[:cout] = bias
    return out


BF16X3_DILATED = os.environ.get("OCCDEPTH_BF16X3_DILATED", "0") == "1"

# Also part of the default ("head") mode since late round 4: the 3x3x3 convolutions with a long K on a SMALL volume (the
# ASPP branches and `mega_context` of the CRP at the 1/8 level: 256 -> 256 / 512 on 32x32x4 = 4096 voxels, K = 27 x 256).
# Too few output tiles to fill 256 CUs, so K2 runs them on its in-workgroup split-K variant at ~96 TF/s of the exact-fp32
# instruction; K2b's split form with the same 4-way split-K (variant 8: M32 x N128, 16 waves) does the MFMA work at 6/16 of
# that instruction's time.  OCCDEPTH_BF16X3_SMALLVOL=0 keeps them on K2.
BF16X3_SMALLVOL = os.environ.get("OCCDEPTH_BF16X3_SMALLVOL", "1") == "1"
SMALLVOL_MAX_VOXELS = 8192
# (1x1x1 convolutions and the CRP products sigmoid(P_logits) @ mega can take the same kernel -- input sigmoid applied while
#  staging -- but do not gain: 512 -> 512 on 4096 rows 78 us against K2's 61, 256 -> 512 27 against 28, 2304 -> 256 75 against
#  78: two MFMA steps per staged chunk.  OCCDEPTH_BF16X3_SMALLVOL_K1=1 routes them there for A/B.)
SMALLVOL_KERNELS = ((3, 3, 3), (1, 1, 1)) if os.environ.get("OCCDEPTH_BF16X3_SMALLVOL_K1", "0") == "1" else ((3, 3, 3),)

# the 8 sub-pixel phases of a stride-2 transposed convolution as one launch (occd_conv3d_fwd_phases); 0 = eight launches
PHASES_ONE_LAUNCH = os.environ.get("OCCDEPTH_PHASES_ONE_LAUNCH", "1") == "1"
# ... and that one launch on K2b with the split (occd_conv3d_bf16_fwd_phases; K2bh or bf16x3 by OCCDEPTH_K2B_SPLIT) instead of
# the exact-fp32 K2, while the split is on at all (OCCDEPTH_BF16X3 != 0): float32-level accuracy, 6/16 of the fp32
# instruction's MFMA time.  0 = K2.
PHASES_X3 = os.environ.get("OCCDEPTH_PHASES_X3", "1") == "1"

# The kernels an eval-path 3-D convolution can take: route -> (weight image it consumes, hip entry point, its flags).
# route() / route_phases() pick one per LAUNCH; DESIGN.md ("3-D convolution routes") has the table with the switches.
K2, K2S3H, K2S3, K2BH, K2B3 = "K2", "K2s3h", "K2s3", "K2bh", "K2b3"
ROUTES = {
    K2: ("f32", "conv3d", {}),                                 # exact fp32
    K2S3H: ("f16x2", "conv3d_f16x2", {}),                      # head, two-term fp16 split
    K2S3: ("x3", "conv3d_bf16", {"split3": True}),             # head, bf16x3 (the entry point picks the sliding-window form)
    K2BH: ("f16x2", "conv3d_bf16", {"f16x2": True}),           # generic kernel, two-term fp16 split
    K2B3: ("x3", "conv3d_bf16", {"split3": True}),             # generic kernel, bf16x3
}
_PACKERS = {"f32": lambda w, s, l: hip.pack_weights(w, s, l), "x3": lambda w, s, l: hip.pack_weights_bf16(w, s, l, split3=True),
            "f16x2": lambda w, s, l: hip.pack_weights_f16x2(w, s, l)}


class PackedW:
    """The weights of one launch (`w`, per-cout `scale`, `layout` as hip.pack_weights) and their packed images by kind
    ("f32" / "x3" / "f16x2"), each packed at the first launch that routes to it.  Warm-up before a graph capture runs the
    same shapes and therefore packs everything the capture needs: the rule that already holds for a plan's `_prepare`.
    The fp16 image needs finite weights on the GPU (its per-channel power-of-two scale; CPU tensors: the emulated path of
    the host-logic tests, which has no fp16 twin); that test -- one host sync -- runs once, at the first launch that asks."""

    def __init__(self, w, scale=None, layout=0):
        self.w, self.scale, self.layout = w, scale, layout
        self.cout, self.cin = (w.shape[1], w.shape[0]) if layout == 2 else (w.shape[0], w.shape[1])
        self.kernel = (1, 1, 1) if layout == 2 else tuple(w.shape[2:])
        self._images = {}
        self._f16x2_ok = None

    def image(self, kind):
        img = self._images.get(kind)
        if img is None:
            img = self._images[kind] = _PACKERS[kind](self.w, self.scale, self.layout)
        return img

    # (plan._wpk.x3: the operand of an explicit hip.conv3d_bf16 / conv3d_phases call, as the tests of the split routes make)
    f32, x3 = property(lambda self: self.image("f32")), property(lambda self: self.image("x3"))

    def f16x2_ok(self):
        if self._f16x2_ok is None:
            w, scale = self.w, self.scale
            self._f16x2_ok = w.is_cuda and bool(torch.isfinite(
                w if scale is None else w * scale.view(-1, *([1] * (w.dim() - 1)))).all())
        return self._f16x2_ok


def _aligned(x):
    return x.cs % 8 == 0 and x.coff % 8 == 0        # K2b stages 8 channels per 16-byte LDS chunk


def _small_volume(x, cout, kernel, **kw):
    """The launch side of the small-volume route: a long K on at most SMALLVOL_MAX_VOXELS output voxels."""
    if kw.get("cin") not in (None, x.C) or x.C < 128 or cout % 128 or not _aligned(x) or x.buf.dtype != torch.float32:
        return False
    pos = kw.get("out_pos")
    if pos is None:
        st, dl, pd = kw.get("stride", (1, 1, 1)), kw.get("dilation", (1, 1, 1)), kw.get("padding", (0, 0, 0))
        pos = tuple((n + 2 * p - d * (k - 1) - 1) // s + 1 for n, p, d, s, k in zip(x.dims, pd, dl, st, kernel))
    return x.batch * pos[0] * pos[1] * pos[2] <= SMALLVOL_MAX_VOXELS and kw.get("tile_hint", 0) == 0


def route(wsrc, x, cout, kernel, out, **kw):
    """The kernel of ONE launch (a key of ROUTES) -- the only reader of BF16X3, HEAD_SPLIT, K2B_SPLIT, BF16X3_SMALLVOL,
    SMALLVOL_KERNELS and BF16X3_DILATED, so a switch takes effect at the next launch.  Each split route wants its weights
    (shape tests on `wsrc`) AND its launch geometry; a route's fp16 form additionally wsrc.f16x2_ok(), else its bf16x3 one."""
    if not BF16X3:
        return K2
    kernel = tuple(kernel)
    head_w = wsrc.layout == 0 and wsrc.kernel == (3, 3, 3) and wsrc.cout <= 32 and 24 < wsrc.cin <= 32
    small_w = (BF16X3_SMALLVOL and wsrc.kernel in SMALLVOL_KERNELS and wsrc.cin >= 128 and wsrc.cin % 16 == 0
               and wsrc.cout % 128 == 0)           # (layout 2, the row operand of gemm_rows, is 1x1x1: opted in with it)
    if BF16X3 != "all" and not (head_w or small_w):
        return K2
    act_in = kw.get("act_in", ACT_NONE)
    if hip.c32x3_eligible(x, cout, kernel, out, **kw):         # the full-resolution head convolutions, all three dilations
        return K2S3H if HEAD_SPLIT == "f16x2" and head_w and wsrc.f16x2_ok() else K2S3
    if BF16X3_SMALLVOL and kernel in SMALLVOL_KERNELS and _small_volume(x, cout, kernel, **kw):   # in-workgroup split-K
        if (K2B_SPLIT == "f16x2" and small_w and wsrc.layout == 0 and kernel == (3, 3, 3) and act_in in (ACT_NONE, ACT_RELU)
                and wsrc.f16x2_ok()):
            return K2BH
        return K2B3
    big = kernel[0] * kernel[1] * kernel[2] >= 8
    if BF16X3 == "all" and _aligned(x) and big and (tuple(kw.get("dilation", (1, 1, 1))) == (1, 1, 1) or BF16X3_DILATED) and \
            kw.get("cin") is None and act_in in (ACT_NONE, ACT_RELU):
        return K2B3                                            # the round-3 experiment: every other large launch
    return K2


def route_phases(phases, x):
    """The kernel of the merged launch of a transposed convolution's sub-pixel phases (`phases`: their PackedW): K2BH, K2B3
    or K2 (exact fp32), or None: one launch per phase, each through route()."""
    if not PHASES_ONE_LAUNCH or len(phases) < 2:
        return None
    if BF16X3 and PHASES_X3 and x.buf.dtype == torch.float32 and _aligned(x):
        return K2BH if K2B_SPLIT == "f16x2" and all(w.f16x2_ok() for w in phases) else K2B3
    return K2 if BF16X3 != "all" else None


def _conv3d(x, wsrc, bias, cout, kernel, out, **kw):
    image, entry, flags = ROUTES[route(wsrc, x, cout, kernel, out, **kw)]
    return getattr(hip, entry)(x, wsrc.image(image), bias, cout, kernel, out, **flags, **kw)


class ConvPlan:
    """conv (+ optional conv bias) + optional BatchNorm3d as one K2 launch."""

    def __init__(self, conv, bn=None, pool=None):
        self.conv, self.bn = conv, bn
        self.pool = _triple(pool) if pool is not None else None  # AvgPool3d(k=stride=pool) in front of a 1x1x1 conv
        self._key = None
        self._wpk = self._bias = None

    @property
    def cout(self):
        return self.conv.out_channels

    def _prepare(self):
        key = _stamp(self.conv, self.bn)
        if key == self._key:
            return
        w = self.conv.weight.detach().float()
        dev = w.device
        cout = self.cout
        scale, shift = _bn_affine(self.bn, cout, dev)
        if self.conv.bias is not None:
            cb = self.conv.bias.detach().float()
            shift = shift + (cb * scale if scale is not None else cb)
        if self.pool is not None:
            # mean over the pooling window then 1x1x1 conv == conv with k = stride = window, w / |window|
            kx, ky, kz = self.pool
            w = (w / float(kx * ky * kz)).expand(-1, -1, kx, ky, kz).contiguous()
        self._wpk = PackedW(w, scale)
        self._bias = _pad_bias(shift, cout)
        self._wrows = None
        if self.pool is None and tuple(w.shape[2:]) == (1, 1, 1) and _triple(self.conv.stride) == (1, 1, 1):
            w2 = w.reshape(cout, -1)
            if ROWS_GEMM and w2.is_cuda and w2.shape[1] % 16 == 0 and cout % 8 == 0:
                self._wrows = hip.RowsGemmWeights((w2 * scale.view(-1, 1) if scale is not None else w2).t().contiguous())
        self._key = key

    def geometry(self):
        if self.pool is not None:
            return self.pool, self.pool, (1, 1, 1), (0, 0, 0)
        c = self.conv
        return _triple(c.kernel_size), _triple(c.stride), _triple(c.dilation), _triple(c.padding)

    def out_dims(self, dims):
        k, s, d, p = self.geometry()
        return tuple((n + 2 * pp - dd * (kk - 1) - 1) // ss + 1 for n, kk, ss, dd, pp in zip(dims, k, s, d, p))

    def __call__(self, x, out=None, res1=None, res2=None, act_in=ACT_NONE, act_out=ACT_NONE):
        self._prepare()
        k, s, d, p = self.geometry()
        if out is None:
            out = Vox.empty(x.batch, self.out_dims(x.dims), self.cout, x.buf.device)
        if (ROWS_GEMM and self._wrows is not None and res2 is None and x.buf.is_cuda and _rows_gemm_wins(x, self._wrows.K)
                and hip.rows_gemm_supported(self._wrows.K, self.cout, x, out, res1)):
            return hip.rows_gemm(x, self._wrows, out, bias=self._bias, res=res1, act_in=act_in, act_out=act_out)
        return _conv3d(x, self._wpk, self._bias, self.cout, k, out, stride=s, dilation=d, padding=p,
                          res1=res1, res2=res2, act_in=act_in, act_out=act_out)


class DerivedConvPlan:
    """A K2 launch whose weights are a function of several modules' parameters (slices / concatenations),
    e.g. the cascade head's merged `conv_classes[:, :planes] | occ_classes` convolution.

    `derive()` returns (weight (Cout, Cin, kx, ky, kz), bias (Cout,) or None); geometry is fixed."""

    def __init__(self, modules, derive, padding=(1, 1, 1), dilation=(1, 1, 1), stride=(1, 1, 1)):
        self.modules, self.derive = list(modules), derive
        self.padding, self.dilation, self.stride = padding, dilation, stride
        self._key = None
        self._wpk = self._bias = None
        self.cout = self.kernel = None

    def _prepare(self):
        key = _stamp(*self.modules)
        if key == self._key:
            return
        w, b = self.derive()
        w = w.detach().float().contiguous()
        self.cout, self.kernel = w.shape[0], tuple(w.shape[2:])
        self._wpk = PackedW(w)
        self._bias = _pad_bias(b.detach().float(), self.cout) if b is not None else None
        self._key = key

    def __call__(self, x, out=None, res1=None, res2=None, act_in=ACT_NONE, act_out=ACT_NONE, out_cs=None):
        self._prepare()
        if out is None:
            dims = tuple((n + 2 * p - d * (k - 1) - 1) // s + 1
                         for n, k, s, d, p in zip(x.dims, self.kernel, self.stride, self.dilation, self.padding))
            out = Vox.empty(x.batch, dims, self.cout, x.buf.device, cs=out_cs)
        return _conv3d(x, self._wpk, self._bias, self.cout, self.kernel, out, stride=self.stride,
                          dilation=self.dilation, padding=self.padding, res1=res1, res2=res2, act_in=act_in,
                          act_out=act_out)


class ConvTransposePlan:
    """ConvTranspose3d(k=3, s=2, p=1, output_padding=1) (+BN) as 8 sub-pixel phase convolutions,
    or ConvTranspose3d(k=3, s=1, p=1) (+BN) as one flipped convolution."""

    def __init__(self, convt, bn=None):
        self.convt, self.bn = convt, bn
        ks, st = _triple(convt.kernel_size), _triple(convt.stride)
        pd, op = _triple(convt.padding), _triple(convt.output_padding)
        if ks != (3, 3, 3) or pd != (1, 1, 1) or _triple(convt.dilation) != (1, 1, 1):
            raise NotImplementedError("only the k3/p1 transposed convolutions of OccDepth are planned")
        if st == (2, 2, 2) and op == (1, 1, 1):
            self.up = 2
        elif st == (1, 1, 1) and op == (0, 0, 0):
            self.up = 1
        else:
            raise NotImplementedError(f"ConvTranspose3d stride {st} output_padding {op}")
        self._key = None
        self._phases = None
        self._bias = None

    @property
    def cout(self):
        return self.convt.out_channels

    def _prepare(self):
        key = _stamp(self.convt, self.bn)
        if key == self._key:
            return
        wt = self.convt.weight.detach().float()  # (Cin, Cout, 3, 3, 3)
        dev = wt.device
        scale, shift = _bn_affine(self.bn, self.cout, dev)
        if self.convt.bias is not None:
            cb = self.convt.bias.detach().float()
            shift = shift + (cb * scale if scale is not None else cb)
        w = wt.permute(1, 0, 2, 3, 4)  # (Cout, Cin, k, k, k), k indexes the scatter offset o = s*i - 1 + k
        phases = []
        if self.up == 1:
            phases.append(((0, 0, 0), (3, 3, 3), (1, 1, 1), PackedW(w.flip(2, 3, 4).contiguous(), scale)))
        else:
            # even outputs (o = 2j) see only k=1 at i=j; odd outputs (o = 2j+1) see k=2 at i=j and k=0 at i=j+1
            taps = ([1], [2, 0])
            for px in (0, 1):
                for py in (0, 1):
                    for pz in (0, 1):
                        sub = w[:, :, taps[px]][:, :, :, taps[py]][:, :, :, :, taps[pz]].contiguous()
                        phases.append(((px, py, pz), tuple(sub.shape[2:]), (0, 0, 0), PackedW(sub, scale)))
        self._phases = phases
        self._bias = _pad_bias(shift, self.cout)
        self._key = key

    def out_dims(self, dims):
        return tuple(n * self.up for n in dims)

    def __call__(self, x, out=None, res1=None, act_out=ACT_NONE):
        self._prepare()
        if out is None:
            out = Vox.empty(x.batch, self.out_dims(x.dims), self.cout, x.buf.device)
        def phase(off, kern, pad, wpk):
            return lambda: _conv3d(x, wpk, self._bias, self.cout, kern, out, padding=pad, res1=res1, act_out=act_out,
                                   out_pos=x.dims, o_stride=(self.up,) * 3, o_off=off)

        merged = route_phases([ph[3] for ph in self._phases], x)
        if merged is not None:
            # one launch for the 8 phases (phase = low bits of blockIdx.y, heaviest tap subset first)
            image, _, flags = ROUTES[merged]
            return hip.conv3d_phases(x, [(wpk.image(image), kern, off) for off, kern, _, wpk in self._phases], self._bias, self.cout,
                                     out, res1=res1, act_out=act_out, out_pos=x.dims, o_stride=(self.up,) * 3, **flags)
        thunks = [phase(*ph) for ph in self._phases]
        if x.buf.is_cuda and len(thunks) > 1:
            run_parallel(thunks)                     # the phases write disjoint voxels of `out`
        else:
            for th in thunks:
                th()
        return out


# K15 (csrc/rows_gemm.hip): 1x1x1 convolutions and the CRP product as a row GEMM whose data operand never touches LDS.
# OFF by default -- measured round 3 (sessions 21-23, profiles/r03_rows_gemm_ab.txt): 512>512 on 4096 rows 55-57 us against
# K2's 63, 256>512 30 against 27, 2304>256 205-216 against 78; the config-2 frame 25.28-25.44 ms against 25.09-25.21.  With
# 256 workgroups on 256 CUs nothing hides the L2 latency of the per-stage weight fetch (3.5 us per 32-k stage for 0.85 us of
# MFMA work); K2's in-workgroup split-K (16 waves) does.  OCCDEPTH_ROWS_GEMM=1 enables it for small volumes / long K.
ROWS_GEMM = os.environ.get("OCCDEPTH_ROWS_GEMM", "0") == "1"


def _rows_gemm_wins(x, K):
    rows = x.batch * x.dims[0] * x.dims[1] * x.dims[2]
    return rows <= 65536 or K >= 256


def pack_rows(b_rows):
    """(K, N) row-major device matrix -> the B operand of `gemm_rows`: the matrix itself for K15, else its PackedW
    (occd_pack_weights layout 2) with the exact-fp32 image packed now, on this stream -- the launches that share the operand
    may run on forked streams (run_parallel).  The opt-in split route packs its own image at its first launch."""
    if ROWS_GEMM and b_rows.is_cuda and b_rows.dtype == torch.float32 and b_rows.shape[0] % 16 == 0 and b_rows.shape[1] % 8 == 0:
        return hip.RowsGemmWeights(b_rows), tuple(b_rows.shape)
    wsrc = PackedW(b_rows, layout=2)
    wsrc.image("f32")
    return wsrc, tuple(b_rows.shape)


def gemm_rows(a, b_rows, out, act_in=ACT_NONE):
    """out[row, :] = act_in(a[row, :K]) @ b_rows[:K, :N] for channels-last Vox a/out (CRP bmm).

    b_rows is a dense (K, N) row-major device matrix (packed on the fly) or the result of `pack_rows`."""
    wpk, (K, N) = b_rows if isinstance(b_rows, tuple) else pack_rows(b_rows)
    if isinstance(wpk, hip.RowsGemmWeights):
        if not hip.rows_gemm_supported(K, N, a, out):
            raise RuntimeError("gemm_rows: operands do not fit the row-GEMM kernel")
        return hip.rows_gemm(a, wpk, out, act_in=act_in)
    return _conv3d(a, wpk, None, N, (1, 1, 1), out, act_in=act_in, cin=K)


# Independent small launches (the 8 sub-pixel phases of a transposed convolution, the ASPP's dilation branches, the CRP's
# relation branches) CAN be issued round-robin on a few side streams forked from -- and joined back into -- the current
# stream (inside a hipGraph capture the fork / join become graph edges); the thunks must not allocate.  Measured round 3
# and NOT adopted: the config-2 frame went from 25.15 ms (one stream) to 25.25 / 26.04 / 25.73 ms with 2 / 3 / 4 streams --
# a branching graph costs more in cross-queue barriers than the overlapped tails give back.  Default 1 = sequential.
PARALLEL_STREAMS = int(os.environ.get("OCCDEPTH_PARALLEL_STREAMS", "1"))
_side_streams = {}


def run_parallel(thunks, width=None):
    width = PARALLEL_STREAMS if width is None else width
    if width < 2 or len(thunks) < 2 or not torch.cuda.is_available():
        for th in thunks:
            th()
        return
    cur = torch.cuda.current_stream()
    key = (cur.device, width)
    if key not in _side_streams:
        _side_streams[key] = [torch.cuda.Stream(device=cur.device) for _ in range(width)]
    pool = _side_streams[key][:min(width, len(thunks))]
    fork = torch.cuda.Event()
    fork.record(cur)
    for s in pool:
        s.wait_event(fork)
    for i, th in enumerate(thunks):
        with torch.cuda.stream(pool[i % len(pool)]):
            th()
    for s in pool:
        cur.wait_stream(s)


def as_vox(x):
    """(B, C, X, Y, Z) tensor -> Vox; zero-copy when it already is a full channels-last buffer of ours."""
    if isinstance(x, Vox):
        return x
    if x.dim() != 5:
        raise RuntimeError("expected a (B, C, X, Y, Z) tensor")
    if not x.is_cuda:
        raise RuntimeError("the HIP path needs GPU tensors (there is no CPU fallback)")
    x = x.float()
    cl = x.permute(0, 2, 3, 4, 1)
    if cl.is_contiguous() and x.shape[1] % 8 == 0:
        return Vox(cl, x.shape[1])
    return Vox.from_ncdhw(x)
