"""ctypes binding of libocc_hip.so (include/occdepth_amd.h).

torch is used here only as the owner of device memory and of the HIP stream:
every function takes torch CUDA(=HIP) tensors, passes raw pointers + sizes
through the C ABI and launches on torch's current stream.  There is NO fallback:
a missing / unloadable library or a CPU tensor raises.
"""
import collections
import ctypes
import os
from ctypes import c_int32, c_int64, c_void_p

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libocc_hip.so")

# Everything the C ABI defines comes from include/occdepth_amd.h through abi.py; the names below are aliases.
EXPORTS = abi.EXPORTS
ABI_VERSION = abi.ABI_VERSION
MAX_VIEWS = abi.CONSTANTS["OCCD_MAX_VIEWS"]
MAX_SCALES = abi.CONSTANTS["OCCD_MAX_SCALES"]
ACT_NONE = abi.CONSTANTS["OCCD_ACT_NONE"]
ACT_RELU = abi.CONSTANTS["OCCD_ACT_RELU"]
ACT_SIGMOID = abi.CONSTANTS["OCCD_ACT_SIGMOID"]
ACT_RELU_PRE = abi.CONSTANTS["OCCD_ACT_RELU_PRE"]
OPTIM_CHUNK = abi.CONSTANTS["OCCD_OPTIM_CHUNK"]   # elements per chunk descriptor
MAX_REGIONS = abi.CONSTANTS["OCCD_MAX_REGIONS"]

Conv3dArgs = abi.STRUCTS["occd_conv3d_args"]
WgradArgs = abi.STRUCTS["occd_conv3d_wgrad_args"]
FlospArgs = abi.STRUCTS["occd_flosp_args"]
LiftArgs = abi.STRUCTS["occd_lift_args"]
LiftProjArgs = abi.STRUCTS["occd_lift_proj_args"]
FlospBwdArgs = abi.STRUCTS["occd_flosp_bwd_args"]
BneckArgs = abi.STRUCTS["occd_bneck_args"]
RowsGemmArgs = abi.STRUCTS["occd_rows_gemm_args"]
GemmArgs = abi.STRUCTS["occd_gemm_args"]
WinoArgs = abi.STRUCTS["occd_wino_args"]
PwArgs = abi.STRUCTS["occd_pw_args"]
LiftBwdArgs = abi.STRUCTS["occd_lift_bwd_args"]
BnArgs = abi.STRUCTS["occd_bn_args"]
FrustumArgs = abi.STRUCTS["occd_frustum_args"]
ConfusionRegion = abi.STRUCTS["occd_confusion_region"]
ConfusionRegionsArgs = abi.STRUCTS["occd_confusion_regions_args"]
Vox2PixArgs = abi.STRUCTS["occd_vox2pix_args"]
OptimChunk = abi.STRUCTS["occd_optim_chunk"]
ClipAdamWArgs = abi.STRUCTS["occd_clip_adamw_args"]
AccumAdamWArgs = abi.STRUCTS["occd_accum_adamw_args"]
RenderView = abi.STRUCTS["OccdRenderView"]
RenderArgs = abi.STRUCTS["OccdRenderArgs"]
StereoArgs = abi.STRUCTS["OccdStereoArgs"]
RENDER_MAX_VIEWS = abi.CONSTANTS["OCCD_RENDER_MAX_VIEWS"]
FuseArgs = abi.STRUCTS["OccdFuseArgs"]
FUSE_MAX_SOURCES = abi.CONSTANTS["OCCD_FUSE_MAX_SOURCES"]
MapFrameArgs = abi.STRUCTS["OccdMapFrameArgs"]
MapExtractArgs = abi.STRUCTS["OccdMapExtractArgs"]
MAP_BRICK = abi.CONSTANTS["OCCD_MAP_BRICK"]
MapRenderArgs = abi.STRUCTS["OccdMapRenderArgs"]
MapSampleArgs = abi.STRUCTS["OccdMapSampleArgs"]
MAP_SAMPLE_EXCLUDE_SELF = abi.CONSTANTS["OCCD_MAP_SAMPLE_EXCLUDE_SELF"]
MAP_SAMPLE_KEEP_OWN = abi.CONSTANTS["OCCD_MAP_SAMPLE_KEEP_OWN"]
MapMergeArgs = abi.STRUCTS["OccdMapMergeArgs"]
VisibilityArgs = abi.STRUCTS["OccdVisibilityArgs"]
MapWeightedArgs = abi.STRUCTS["OccdMapWeightedArgs"]
MapSampleWeightedArgs = abi.STRUCTS["OccdMapSampleWeightedArgs"]
RayMetricArgs = abi.STRUCTS["OccdRayMetricArgs"]
RAY_MAX_THRESHOLDS = abi.CONSTANTS["OCCD_RAY_MAX_THRESHOLDS"]
RAY_MAX_CLASSES = abi.CONSTANTS["OCCD_RAY_MAX_CLASSES"]
RAY_UNKNOWN_DROP = abi.CONSTANTS["OCCD_RAY_UNKNOWN_DROP"]
RAY_UNKNOWN_PASS = abi.CONSTANTS["OCCD_RAY_UNKNOWN_PASS"]
RAY_COUNTERS = abi.CONSTANTS["OCCD_RAY_COUNTERS"]
RenderLossArgs = abi.STRUCTS["OccdRenderLossArgs"]
RENDER_LOSS_ABS = abi.CONSTANTS["OCCD_RENDER_LOSS_ABS"]
RENDER_LOSS_REL = abi.CONSTANTS["OCCD_RENDER_LOSS_REL"]
EdtArgs = abi.STRUCTS["OccdEdtArgs"]
EDT_MAX_CLASSES = abi.CONSTANTS["OCCD_EDT_MAX_CLASSES"]
EDT_CHUNK = abi.CONSTANTS["OCCD_EDT_CHUNK"]
EDT_MAX_D2 = 65534
SortArgs = abi.STRUCTS["OccdSortArgs"]
SORT_TILE = abi.CONSTANTS["OCCD_SORT_TILE"]
SORT_RADIX_BITS = abi.CONSTANTS["OCCD_SORT_RADIX_BITS"]
LovaszArgs = abi.STRUCTS["OccdLovaszArgs"]
LOVASZ_Q = abi.CONSTANTS["OCCD_LOVASZ_Q"]
LOVASZ_KEY_BITS = abi.CONSTANTS["OCCD_LOVASZ_KEY_BITS"]
LOVASZ_INVALID_KEY = abi.CONSTANTS["OCCD_LOVASZ_INVALID_KEY"]
LOVASZ_RANK_TILE = abi.CONSTANTS["OCCD_LOVASZ_RANK_TILE"]
MeshArgs = abi.STRUCTS["OccdMeshArgs"]
MESH_MAX_GRID = abi.CONSTANTS["OCCD_MESH_MAX_GRID"]
MESH_MAX_CELLS = abi.CONSTANTS["OCCD_MESH_MAX_CELLS"]
MESH_MAX_KEY_BITS = abi.CONSTANTS["OCCD_MESH_MAX_KEY_BITS"]
CclArgs = abi.STRUCTS["OccdCclArgs"]
CclPairArgs = abi.STRUCTS["OccdCclPairArgs"]
CCL_TILE = abi.CONSTANTS["OCCD_CCL_TILE"]
CCL_NO_TILE_PASS = abi.CONSTANTS["OCCD_CCL_NO_TILE_PASS"]
CCL_STATUS_OVERRUN = abi.CONSTANTS["OCCD_CCL_STATUS_OVERRUN"]
CCL_STATUS_INSTANCE = abi.CONSTANTS["OCCD_CCL_STATUS_INSTANCE"]
ProfRow = abi.STRUCTS["occd_prof_row"]


_lib = None
_PROFILING = False


def load():
    """Load libocc_hip.so (raises if it has not been built: there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m occdepth_amd.build` "
            "(the MI355X HIP kernels are the only implementation of this path)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.occd_abi_version() != ABI_VERSION:
        raise RuntimeError("libocc_hip.so ABI version mismatch; rebuild it")
    _lib = lib
    return lib


def _check(code, what):
    if code != 0:
        msg = load().occd_strerror(code).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {code})")


def _ptr(t, name="tensor"):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (the HIP kernels have no CPU path)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t.data_ptr()


def _f32(t, name):
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    return _ptr(t, name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------- voxel tensors
class Vox:
    """Channels-last voxel tensor view: buf is (B, X, Y, Z, cs) float32 (bfloat16 for the bf16-storage variants of
    K2b / K8b); the logical tensor is buf[..., coff:coff+C].  Pads in [C, round8(C)) must be zero."""

    __slots__ = ("buf", "C", "coff")

    def __init__(self, buf, C, coff=0):
        assert buf.dim() == 5 and buf.dtype in (torch.float32, torch.bfloat16)
        self.buf, self.C, self.coff = buf, int(C), int(coff)

    @property
    def cs(self):
        return self.buf.shape[4]

    @property
    def dims(self):
        return tuple(self.buf.shape[1:4])

    @property
    def batch(self):
        return self.buf.shape[0]

    def ncdhw(self):
        """Logical (B, C, X, Y, Z) view (channels_last_3d strides, no copy)."""
        return self.buf[..., self.coff:self.coff + self.C].permute(0, 4, 1, 2, 3)

    @staticmethod
    def empty(batch, dims, C, device, cs=None, dtype=torch.float32):
        cs = cs if cs is not None else round_up(C, 8)
        return Vox(torch.empty((batch,) + tuple(dims) + (cs,), device=device, dtype=dtype), C)

    @staticmethod
    def from_ncdhw(x):
        """(B, C, X, Y, Z) float32 -> channels-last Vox with zeroed channel pad (HIP transpose)."""
        B, C = x.shape[0], x.shape[1]
        dims = tuple(x.shape[2:])
        v = Vox.empty(B, dims, C, x.device)
        xc = x.contiguous()
        S = dims[0] * dims[1] * dims[2]
        _check(load().occd_nchw_to_nhwc(_f32(xc, "x"), _f32(v.buf, "out"), B, C, S, v.cs, _stream()),
               "occd_nchw_to_nhwc")
        return v


def round_up(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------------------- K2
def packed_weight_floats(cout, cin, taps):
    n = load().occd_packed_weight_floats(cout, cin, taps)
    if n <= 0:
        raise RuntimeError("occd_packed_weight_floats: bad shape")
    return n


def _weight_geometry(w, layout):
    """(cout, cin, kernel) of a weight tensor: (Cout, Cin, kx, ky, kz), or [layout 2] a (K, N) row-major GEMM B operand."""
    if layout == 2:
        cin, cout = w.shape
        return cout, cin, (1, 1, 1)
    return w.shape[0], w.shape[1], tuple(w.shape[2:])


def pack_weights(w, scale=None, layout=0):
    """w: (Cout, Cin, kx, ky, kz) [layout 0] / (K, N) row-major GEMM B operand [layout 2]."""
    cout, cin, k = _weight_geometry(w, layout)
    w = w.contiguous()
    out = torch.empty(packed_weight_floats(cout, cin, k[0] * k[1] * k[2]), device=w.device, dtype=torch.float32)
    sc = scale.contiguous() if scale is not None else None
    _check(load().occd_pack_weights(_f32(w, "w"), _f32(sc, "scale") if sc is not None else None,
                                    _f32(out, "wpk"), cout, cin, k[0], k[1], k[2], layout, _stream()),
           "occd_pack_weights")
    return out


def pack_weights_gather(w, cout, cin, s_co, s_ci, tap_ofs, kernel=None, bf16=False):
    """Packed image of the operator W'[co][ci][tap] = w.flat[co * s_co + ci * s_ci + tap_ofs[tap]] (a transposed / flipped /
    tap-subset view of the dense float32 tensor `w`) for `conv3d` (bf16=False) or `conv3d_bf16`; one launch, no temporaries.
    `kernel` (the (kx, ky, kz) the taps enumerate) is only read by the CPU emulation."""
    if w.dtype != torch.float32 or not w.is_contiguous():
        raise RuntimeError("pack_weights_gather needs a contiguous float32 source tensor")
    n = len(tap_ofs)
    ofs = (c_int32 * n)(*[int(o) for o in tap_ofs])
    if max(ofs) + (cout - 1) * s_co + (cin - 1) * s_ci >= w.numel():
        raise RuntimeError("pack_weights_gather: view exceeds the source tensor")
    if bf16 == "x3":                       # hi | mid | lo images for conv3d_bf16(..., split3=True)
        out = torch.empty(3 * load().occd_packed_weight_bf16_elems(cout, cin, n), device=w.device, dtype=torch.bfloat16)
        _check(load().occd_pack_weights_bf16x3_gather(_f32(w, "w"), None, _ptr(out, "wpk"), cout, cin, n, s_co, s_ci,
                                                      ctypes.cast(ofs, c_void_p), _stream()), "occd_pack_weights_bf16x3_gather")
    elif bf16:
        out = torch.empty(load().occd_packed_weight_bf16_elems(cout, cin, n), device=w.device, dtype=torch.bfloat16)
        _check(load().occd_pack_weights_bf16_gather(_f32(w, "w"), None, _ptr(out, "wpk"), cout, cin, n, s_co, s_ci,
                                                    ctypes.cast(ofs, c_void_p), _stream()), "occd_pack_weights_bf16_gather")
    else:
        out = torch.empty(packed_weight_floats(cout, cin, n), device=w.device, dtype=torch.float32)
        _check(load().occd_pack_weights_gather(_f32(w, "w"), None, _f32(out, "wpk"), cout, cin, n, s_co, s_ci,
                                               ctypes.cast(ofs, c_void_p), _stream()), "occd_pack_weights_gather")
    return out


def _conv3d_args(x, wpk_ptr, bias, cout, kernel, out, stride, dilation, padding, res1, res2, act_in, act_out, out_pos,
                 o_stride, o_off, cin, tile_hint, ptr):
    a = Conv3dArgs()
    a.inp, a.wpk = ptr(x.buf, "x"), wpk_ptr
    a.bias = _f32(bias, "bias") if bias is not None else None
    a.res1 = ptr(res1.buf, "res1") if res1 is not None else None
    a.res2 = ptr(res2.buf, "res2") if res2 is not None else None
    a.out = ptr(out.buf, "out")
    a.batch = x.batch
    a.X, a.Y, a.Z = x.dims
    a.cin = x.C if cin is None else cin
    a.in_cs, a.in_coff = x.cs, x.coff
    a.cout, a.out_cs, a.out_coff = cout, out.cs, out.coff
    if res1 is not None:
        a.res1_cs, a.res1_coff = res1.cs, res1.coff
    if res2 is not None:
        a.res2_cs, a.res2_coff = res2.cs, res2.coff
    a.kx, a.ky, a.kz = kernel
    a.sx, a.sy, a.sz = stride
    a.dx, a.dy, a.dz = dilation
    a.px, a.py, a.pz = padding
    a.OX, a.OY, a.OZ = out.dims
    if out_pos is None:
        out_pos = tuple((n + 2 * p - d * (k - 1) - 1) // s + 1
                        for n, p, d, k, s in zip(x.dims, padding, dilation, kernel, stride))
    a.Xo, a.Yo, a.Zo = out_pos
    a.o_stride_x, a.o_stride_y, a.o_stride_z = o_stride
    a.o_off_x, a.o_off_y, a.o_off_z = o_off
    a.act_in, a.act_out = act_in, act_out
    a.cout_store = min(round_up(cout, 8), out.cs - out.coff, round_up(cout, 32))
    a.tile_hint = tile_hint
    if _PROFILING:
        set_tag("%d>%d k%d%d%d s%d%d%d d%d%d%d @%dx%dx%d" % ((a.cin, a.cout) + tuple(kernel) + tuple(stride)
                                                              + tuple(dilation) + tuple(x.dims)))
    return a


def conv3d(x, wpk, bias, cout, kernel, out, stride=(1, 1, 1), dilation=(1, 1, 1), padding=(0, 0, 0),
           res1=None, res2=None, act_in=ACT_NONE, act_out=ACT_NONE, out_pos=None, o_stride=(1, 1, 1),
           o_off=(0, 0, 0), cin=None, tile_hint=0):
    """out = act_out(conv(act_in(x)) + bias + res1 + res2) on Vox tensors (see include/occdepth_amd.h)."""
    a = _conv3d_args(x, _f32(wpk, "wpk"), bias, cout, kernel, out, stride, dilation, padding, res1, res2, act_in, act_out,
                     out_pos, o_stride, o_off, cin, tile_hint, _f32)
    _check(load().occd_conv3d_fwd(ctypes.byref(a), _stream()), "occd_conv3d_fwd")
    return out


def conv3d_phases(x, phases, bias, cout, out, res1=None, act_out=ACT_NONE, out_pos=None, o_stride=(1, 1, 1), split3=False,
                  f16x2=False):
    """The sub-pixel phases of one transposed convolution as ONE launch: K2 (occd_conv3d_fwd_phases) or, split3, K2b with the
    3-way bf16 split (occd_conv3d_bf16_fwd_phases), or, f16x2, K2bh: K2b with the two-term fp16 split.
    phases: 1 / 2 / 4 / 8 tuples (wpk, kernel, o_off) -- the packed weights of the phase's tap subset (pack_weights,
    pack_weights_bf16(split3=True) or pack_weights_f16x2), its extent and where its voxels land in `out`; padding 0, stride /
    dilation 1, everything else shared."""
    mode = _split_mode("conv3d_phases", split3, f16x2)
    if mode is not None:
        error = ("conv3d_phases(f16x2=True) needs the images of pack_weights_f16x2" if f16x2 else
                 "conv3d_phases(split3=True) needs the images of pack_weights_bf16(split3=True)")
        return _conv3d_bf16_pipe(mode, error, x, phases, bias, cout, out, merged=True, res1=res1, act_out=act_out, out_pos=out_pos,
                                 o_stride=o_stride)
    n = len(phases)
    arr = (Conv3dArgs * n)()
    for i, (wpk, kernel, o_off) in enumerate(phases):
        arr[i] = _conv3d_args(x, _f32(wpk, "wpk"), bias, cout, kernel, out, (1, 1, 1), (1, 1, 1), (0, 0, 0), res1, None, ACT_NONE,
                              act_out, out_pos, o_stride, o_off, None, 0, _f32)
    _tag_phases(x, cout, n)
    _check(load().occd_conv3d_fwd_phases(arr, n, _stream()), "occd_conv3d_fwd_phases")
    return out


def _tag_phases(x, cout, n):
    if _PROFILING:
        set_tag("%d>%d k333 s222 transposed: %d phases @%dx%dx%d" % ((x.C, cout, n) + tuple(x.dims)))


# ----------------------------------------------------------------------------- K2b / K8b (bf16 MFMA)
def _act_ptr(dtype):
    def ptr(t, name):
        if t.dtype != dtype:
            raise RuntimeError(f"{name} must be {dtype} like the other activation tensors of the launch, got {t.dtype}")
        return _ptr(t, name)
    return ptr


# the `dtype` argument of occd_conv3d_bf16_fwd[_phases] (include/occdepth_amd.h)
CONV_F32, CONV_BF16, CONV_BF16X3, CONV_F16X2_HEAD, CONV_F16X2 = (
    abi.CONSTANTS["OCCD_CONV_" + n] for n in ("F32", "BF16", "BF16X3", "F16X2_HEAD", "F16X2"))
# mode -> (dtype of its weight image, the error when the activation tensors are not float32 / None: they pick the mode)
_CONV_MODES = {
    CONV_F32: (torch.bfloat16, None), CONV_BF16: (torch.bfloat16, None),
    CONV_BF16X3: (torch.bfloat16, "the 3-way split takes float32 tensors"),
    CONV_F16X2_HEAD: (torch.uint8, "the fp16 split takes float32 tensors"),
    CONV_F16X2: (torch.uint8, "the fp16 split takes float32 tensors"),
}


def _storage_code(dtype):
    if dtype == torch.float32:
        return CONV_F32
    if dtype == torch.bfloat16:
        return CONV_BF16
    raise RuntimeError(f"the bf16-MFMA kernels take float32 or bfloat16 activations, got {dtype}")


def _split_mode(who, split3, f16x2):
    """The mode of the public flags: CONV_F16X2 / CONV_BF16X3, or None when neither is set."""
    if split3 and f16x2:
        raise RuntimeError(f"{who}: split3 and f16x2 are two forms of one launch, pick one")
    return CONV_F16X2 if f16x2 else CONV_BF16X3 if split3 else None


def _conv3d_bf16_pipe(mode, image_error, x, phases, bias, cout, out, merged=False, stride=(1, 1, 1), dilation=(1, 1, 1),
                      padding=(0, 0, 0), res1=None, res2=None, act_in=ACT_NONE, act_out=ACT_NONE, out_pos=None, o_stride=(1, 1, 1),
                      cin=None, tile_hint=0):
    """The one launcher of the bf16-pipe entry points in `mode` (a CONV_* constant): occd_conv3d_bf16_fwd on the single
    (wpk, kernel, o_off) of `phases`, or, merged, occd_conv3d_bf16_fwd_phases on all of them."""
    image_dtype, f32_only = _CONV_MODES[mode]
    if any(wpk.dtype != image_dtype for wpk, _, _ in phases):
        raise RuntimeError(image_error)
    if f32_only and x.buf.dtype != torch.float32:
        raise RuntimeError(f32_only)
    ptr = _act_ptr(x.buf.dtype)
    n = len(phases)
    arr = (Conv3dArgs * n)()
    for i, (wpk, kernel, o_off) in enumerate(phases):
        arr[i] = _conv3d_args(x, _ptr(wpk, "wpk"), bias, cout, kernel, out, stride, dilation, padding, res1, res2, act_in, act_out,
                              out_pos, o_stride, o_off, cin, tile_hint, ptr)
    if merged:
        _tag_phases(x, cout, n)
        _check(load().occd_conv3d_bf16_fwd_phases(arr, n, mode, _stream()), "occd_conv3d_bf16_fwd_phases")
    else:
        _check(load().occd_conv3d_bf16_fwd(arr, mode, _stream()),
               "occd_conv3d_bf16_fwd" + (" (f16x2)" if image_dtype == torch.uint8 else ""))
    return out


def pack_weights_bf16(w, scale=None, layout=0, split3=False):
    """fp32 master weights -> the bf16 fragment image of K2b (shapes / layouts as `pack_weights`); split3: the three images
    hi | mid | lo of the 3-way split experiment (conv3d_bf16(..., split3=True))."""
    cout, cin, k = _weight_geometry(w, layout)
    w = w.detach().float().contiguous()
    n = load().occd_packed_weight_bf16_elems(cout, cin, k[0] * k[1] * k[2])
    if n <= 0:
        raise RuntimeError("occd_packed_weight_bf16_elems: bad shape")
    out = torch.empty(3 * n if split3 else n, device=w.device, dtype=torch.bfloat16)
    sc = scale.detach().float().contiguous() if scale is not None else None
    fn = load().occd_pack_weights_bf16x3 if split3 else load().occd_pack_weights_bf16
    _check(fn(_f32(w, "w"), _f32(sc, "scale") if sc is not None else None, _ptr(out, "wpk"),
              cout, cin, k[0], k[1], k[2], layout, _stream()), "occd_pack_weights_bf16")
    return out


def pack_weights_f16x2(w, scale=None, layout=0):
    """fp32 master weights -> the image of K2s3h and K2bh, the two-term fp16 split (conv3d_f16x2 for the head convolutions,
    conv3d_bf16 / conv3d_phases(..., f16x2=True) for any other geometry): three fp16
    images hi | hs | lo of the per-channel power-of-two scaled weights plus the epilogue factors (a uint8 tensor of
    occd_packed_weight_f16x2_bytes bytes).  The weights must be finite."""
    cout, cin, k = _weight_geometry(w, layout)
    w = w.detach().float().contiguous()
    n = load().occd_packed_weight_f16x2_bytes(cout, cin, k[0] * k[1] * k[2])
    if n <= 0:
        raise RuntimeError("occd_packed_weight_f16x2_bytes: bad shape")
    out = torch.empty(n, device=w.device, dtype=torch.uint8)
    sc = scale.detach().float().contiguous() if scale is not None else None
    _check(load().occd_pack_weights_f16x2(_f32(w, "w"), _f32(sc, "scale") if sc is not None else None, _ptr(out, "wpk"),
                                          cout, cin, k[0], k[1], k[2], layout, _stream()), "occd_pack_weights_f16x2")
    return out


def conv3d_f16x2(x, wpk, bias, cout, kernel, out, o_off=(0, 0, 0), **kw):
    """K2s3h: `conv3d` of a full-resolution head convolution (`c32x3_eligible`) with the two-term fp16 split of both
    operands (float32 tensors, wpk = pack_weights_f16x2(w)).  Other geometries are an error: there is no generic form."""
    return _conv3d_bf16_pipe(CONV_F16X2_HEAD, "conv3d_f16x2 needs the image of pack_weights_f16x2", x, [(wpk, kernel, o_off)],
                             bias, cout, out, **kw)


def set_head_lo(form):
    """Where K2s3h (`conv3d_f16x2`) takes the lo weight image from: 1 (the default) resident in LDS beside hi, hs = hi 2^-11
    formed in registers; 0 the form before (hi | hs in LDS, lo streamed from L2 through a register ring).  Bit-identical
    outputs.  Returns the previous setting; anything but 0 / 1 is refused."""
    if isinstance(form, bool) or not isinstance(form, int) or form not in (0, 1):
        raise ValueError(f"set_head_lo: 0 (ring) or 1 (LDS), got {form!r}")
    return load().occd_conv3d_head_set_lo(form)


def conv3d_bf16(x, wpk, bias, cout, kernel, out, stride=(1, 1, 1), dilation=(1, 1, 1), padding=(0, 0, 0),
                res1=None, res2=None, act_in=ACT_NONE, act_out=ACT_NONE, out_pos=None, o_stride=(1, 1, 1),
                o_off=(0, 0, 0), cin=None, tile_hint=0, split3=False, f16x2=False):
    """K2b: `conv3d` on the bf16 matrix pipe (fp32 accumulate).  x / out / res1 / res2 are all float32 Vox tensors
    (converted to bf16 while staging) or all bfloat16 ones; wpk = pack_weights_bf16(w).
    split3 (float32 tensors, wpk = pack_weights_bf16(w, split3=True)): the 3-way split experiment, float32-level accuracy.
    f16x2 (float32 tensors, wpk = pack_weights_f16x2(w), act_in none / relu): K2bh, the same kernel on the f16 matrix pipe with
    the two-term fp16 split -- K2s3h's numerics at any geometry; finite |x| >= 32760 overflow to non-finite outputs."""
    mode = _split_mode("conv3d_bf16", split3, f16x2)
    error = ("conv3d_bf16(f16x2=True) needs the image of pack_weights_f16x2" if f16x2 else
             "conv3d_bf16 needs the bf16 weight image of pack_weights_bf16")
    if mode is None:
        mode = _storage_code(x.buf.dtype)
    return _conv3d_bf16_pipe(mode, error, x, [(wpk, kernel, o_off)], bias, cout, out, stride=stride,
                             dilation=dilation, padding=padding, res1=res1, res2=res2, act_in=act_in, act_out=act_out,
                             out_pos=out_pos, o_stride=o_stride, cin=cin, tile_hint=tile_hint)


GEMM_ACT = {None: abi.CONSTANTS["OCCD_GEMM_ACT_NONE"], "none": abi.CONSTANTS["OCCD_GEMM_ACT_NONE"],
            "swish": abi.CONSTANTS["OCCD_GEMM_ACT_SWISH"], "leaky": abi.CONSTANTS["OCCD_GEMM_ACT_LEAKY"]}


GEMM_PRE_F16X2 = abi.CONSTANTS["OCCD_GEMM_PRE_F16X2"]


class GemmPacked:
    """A static GEMM operand (weights) split once into its three bf16 terms in MFMA fragment order (occd_gemm_x3_pack):
    role "a" = the left operand (M, K) / (batch, M, K), role "b" = the right operand (K, N) / (batch, K, N).
    split="f16x2" (role "a" only): the image of occd_gemm_f16x2_pack instead -- rows scaled by powers of two, two fp16 terms,
    the row factors behind them -- which K16p, K21 and K16's pre-split form multiply with three fp16 MFMAs per K step (the
    numerics of the head convolutions; finite |b| >= 32760 overflow).  Raises ValueError when a weight is not finite: such a
    matrix has no f16x2 image."""

    def __init__(self, w, role, split="bf16x3"):
        if role not in ("a", "b") or w.dim() not in (2, 3) or w.dtype != torch.float32 or not w.is_cuda:
            raise RuntimeError("GemmPacked: a 2-D / 3-D float32 GPU tensor and role 'a' or 'b'")
        if split not in ("bf16x3", "f16x2") or (split == "f16x2" and role != "a"):
            raise RuntimeError("GemmPacked: split is 'bf16x3', or 'f16x2' with role 'a'")
        w = w.detach().contiguous()
        self.role, self.batch, self.split = role, (w.shape[0] if w.dim() == 3 else None), split
        if role == "a":
            self.rows, self.K = w.shape[-2], w.shape[-1]
        else:
            self.K, self.rows = w.shape[-2], w.shape[-1]
        self.shape = tuple(w.shape)
        if split == "f16x2":
            self.per = load().occd_gemm_f16x2_packed_elems(self.rows, self.K)
            if self.per <= 0:
                raise RuntimeError("occd_gemm_f16x2_packed_elems: bad shape")
            nb = self.batch or 1
            self.buf = torch.empty(nb * self.per, device=w.device, dtype=torch.float16)
            rc = load().occd_gemm_f16x2_pack(w.data_ptr(), self.buf.data_ptr(), self.rows, self.K, w.shape[-1], nb,
                                             w.shape[-2] * w.shape[-1], _stream())
            if rc == abi.CONSTANTS["OCCD_EINVAL"]:
                raise ValueError("occd_gemm_f16x2_pack: a weight is not finite")
            _check(rc, "occd_gemm_f16x2_pack")
            return
        self.per = load().occd_gemm_x3_packed_elems(self.rows, self.K)
        if self.per <= 0:
            raise RuntimeError("occd_gemm_x3_packed_elems: bad shape")
        nb = self.batch or 1
        self.buf = torch.empty(nb * self.per, device=w.device, dtype=torch.bfloat16)
        _check(load().occd_gemm_x3_pack(w.data_ptr(), self.buf.data_ptr(), self.rows, self.K, w.shape[-1], 0 if role == "a" else 1,
                                        nb, w.shape[-2] * w.shape[-1], _stream()), "occd_gemm_x3_pack")

    def dim(self):
        return len(self.shape)


def gemm_x3_supported(a, b):
    """Shapes / layouts K16 takes: a (M, K) or (batch, M, K), b (batch, K, N) or (K, N); float32, innermost stride 1,
    K % 8 == 0, 16-byte aligned rows of a, N >= 4.  Either operand may be a `GemmPacked` (pre-split weights)."""
    if isinstance(a, GemmPacked) and isinstance(b, GemmPacked):
        return False
    for t, role in ((a, "a"), (b, "b")):
        if isinstance(t, GemmPacked):
            if t.role != role:
                return False
        elif t.dtype != torch.float32 or not t.is_cuda or t.dim() not in (2, 3) or t.stride(-1) != 1:
            return False
    K = a.K if isinstance(a, GemmPacked) else a.shape[-1]
    Kb = b.K if isinstance(b, GemmPacked) else b.shape[-2]
    N = b.rows if isinstance(b, GemmPacked) else b.shape[-1]
    if K != Kb or K % 8 or N < 4:
        return False
    if not isinstance(a, GemmPacked):
        if a.stride(-2) % 4 or a.stride(-2) < K or a.data_ptr() % 16 or (a.dim() == 3 and a.stride(0) % 4):
            return False
    if not isinstance(b, GemmPacked) and b.stride(-2) < N:
        return False
    nb_a = (a.batch if isinstance(a, GemmPacked) else (a.shape[0] if a.dim() == 3 else None))
    nb_b = (b.batch if isinstance(b, GemmPacked) else (b.shape[0] if b.dim() == 3 else None))
    return nb_a is None or nb_b is None or nb_a == nb_b


def _gemm_args(who, a, b, out, M, N, K, batch, bias, act, slope, res, k_scale):
    """The occd_gemm_args that K16 and K21 share: operand addresses, sizes, the output's strides and the epilogue operands
    (checked); the operand strides, tile_hint and pre are the caller's."""
    q = GemmArgs()
    q.A, q.B, q.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    if bias is not None:
        if bias.numel() != M or not bias.is_contiguous():
            raise RuntimeError(who + ": bias must be M contiguous floats")
        q.bias = _f32(bias, "bias")
    q.M, q.N, q.K, q.batch = M, N, K, batch
    q.ldc, q.stride_c = out.stride(-2), (out.stride(0) if out.dim() == 3 else 0)
    q.act, q.slope = GEMM_ACT[act], slope
    if res is not None:
        if res.dtype != torch.float32 or res.shape != out.shape or res.stride() != out.stride():
            raise RuntimeError(who + ": res must be laid out like out")
        q.res = res.data_ptr()
    if k_scale is not None:
        if k_scale.dtype != torch.float32 or tuple(k_scale.shape) != (batch, K) or not k_scale.is_contiguous():
            raise RuntimeError(who + ": k_scale must be (batch, K) contiguous floats")
        q.scale_k = k_scale.data_ptr()
    return q


def gemm_x3(a, b, bias=None, act=None, slope=0.01, out=None, tile_hint=0, plain_bf16=False, res=None, k_scale=None,
            sigmoid_a=False, bias_n=None):
    """K16 (occd_gemm_f32x3): out[i] = act(a[i] @ (b[i] * k_scale[i][:, None]) + bias[:, None]) + res[i] in float32-level
    accuracy on the bf16 matrix pipe (k_scale: (batch, K), the squeeze-excite gate of a project convolution; res: laid out
    like out, the block's skip connection).
    a: (M, K) shared over the batch, or (batch, M, K); b: (K, N) or (batch, K, N); out: (batch, M, N) ((M, N) when neither
    operand is batched).  Tensor operands may be strided views as long as the innermost stride is 1; a static operand may be
    given as `GemmPacked(w, "a" / "b")` (split once, read straight from L2).  plain_bf16: operands rounded to ONE bf16 term
    (the bf16 training mode: bf16 MFMA, fp32 storage and accumulate) instead of the split.  sigmoid_a: a -> sigmoid(a) while
    it is staged (the CRP's relation products)."""
    if not gemm_x3_supported(a, b):
        raise RuntimeError("gemm_x3: unsupported operands")
    pa, pb = isinstance(a, GemmPacked), isinstance(b, GemmPacked)
    nb_a = a.batch if pa else (a.shape[0] if a.dim() == 3 else None)
    nb_b = b.batch if pb else (b.shape[0] if b.dim() == 3 else None)
    batch = nb_a or nb_b or 1
    M = a.rows if pa else a.shape[-2]
    K = a.K if pa else a.shape[-1]
    N = b.rows if pb else b.shape[-1]
    squeeze = nb_a is None and nb_b is None
    dev = a.buf.device if pa else a.device
    if out is None:
        out = torch.empty((batch, M, N), device=dev, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.stride(-1) != 1 or out.shape[-2:] != (M, N) or not out.is_cuda:
        raise RuntimeError("gemm_x3: bad output tensor")
    elif not ((out.dim() == 3 and out.shape[0] == batch) or (out.dim() == 2 and squeeze)):
        # the kernel trusts (batch, stride_c): a (1, M, N) or 2-D `out` under a batched operand would be written past its
        # end / once per batch item on top of itself
        raise RuntimeError("gemm_x3: out must be (batch, M, N) with batch = %d (2-D only when neither operand is batched)"
                           % batch)
    q = _gemm_args("gemm_x3", a.buf if pa else a, b.buf if pb else b, out, M, N, K, batch, bias, act, slope, res, k_scale)
    q.lda = K if pa else a.stride(-2)                    # (strided views: the strides travel as lda / ldb / ldc)
    q.ldb = N if pb else b.stride(-2)
    q.stride_a = (a.per if nb_a else 0) if pa else (a.stride(0) if a.dim() == 3 else 0)
    q.stride_b = (b.per if nb_b else 0) if pb else (b.stride(0) if b.dim() == 3 else 0)
    q.tile_hint = tile_hint
    f16x2 = pa and a.split == "f16x2"
    q.pre = (GEMM_PRE_F16X2 if f16x2 else 1) if pa else 2 if pb else (3 if plain_bf16 else 0)
    if plain_bf16 and (pa or pb):
        raise RuntimeError("gemm_x3: plain_bf16 takes float32 tensor operands")
    if f16x2 and bias_n is not None:
        raise RuntimeError("gemm_x3: an f16x2 image takes no column bias")
    if k_scale is not None and pb:
        raise RuntimeError("gemm_x3: k_scale must be (batch, K) contiguous floats and b a float32 tensor")
    if sigmoid_a:
        if pa or plain_bf16:
            raise RuntimeError("gemm_x3: sigmoid_a takes a float32 tensor A and the split arithmetic")
        q.act_a = 1
    if bias_n is not None:                                   # one value per COLUMN: (N,) shared or (batch, N)
        if bias_n.dtype != torch.float32 or not bias_n.is_cuda or not bias_n.is_contiguous() or \
                tuple(bias_n.shape) not in ((N,), (batch, N)):
            raise RuntimeError("gemm_x3: bias_n must be (N,) or (batch, N) contiguous floats")
        q.bias_n, q.stride_bias_n = bias_n.data_ptr(), (N if bias_n.dim() == 2 else 0)
    if _PROFILING:
        set_tag("%dx%dx%d b%d%s" % (M, N, K, batch, " f16x2" if f16x2 else ""))
    _check(load().occd_gemm_f32x3(ctypes.byref(q), _stream()), "occd_gemm_f32x3")
    return out[0] if squeeze and out.dim() == 3 else out


def gemm_x3_splitk_plan(M, N, K, batch):
    """(k16_per_z, nz, row_ranges, workspace_floats) the library proposes for K21 on this problem."""
    per, nz, rr, ws = c_int32(), c_int32(), c_int32(), c_int64()
    _check(load().occd_gemm_f32x3_splitk_plan(M, N, K, batch, ctypes.byref(per), ctypes.byref(nz), ctypes.byref(rr),
                                              ctypes.byref(ws)), "occd_gemm_f32x3_splitk_plan")
    return per.value, nz.value, rr.value, ws.value


_SPLITK_WS = {}        # device -> workspace tensor (grown on demand; stream-ordered reuse: the reduce launch follows its GEMM)


def gemm_x3_splitk(a, b, bias=None, act=None, slope=0.01, out=None, res=None, k_scale=None, plan=None):
    """K21 (occd_gemm_f32x3_splitk): out[i] = act(a @ (b[i] * k_scale[i][:, None]) + bias[:, None]) + res[i] for SKINNY long-K
    problems (the MBConv project convolutions of the 1/16 and 1/32 stages): K cut over the grid, float32 partial tiles in a
    workspace, deterministic second launch.  a: GemmPacked role "a" (shared over the batch); b: (batch, K, N) / (K, N)
    float32, innermost stride 1; plan: (k16_per_z, nz, row_ranges) or None for the library's proposal."""
    if not isinstance(a, GemmPacked) or a.role != "a" or a.batch is not None:
        raise RuntimeError("gemm_x3_splitk: a must be a shared GemmPacked left operand")
    if b.dtype != torch.float32 or not b.is_cuda or b.dim() not in (2, 3) or b.stride(-1) != 1:
        raise RuntimeError("gemm_x3_splitk: b must be a float32 GPU tensor with innermost stride 1")
    batch = b.shape[0] if b.dim() == 3 else 1
    M, K, N = a.rows, a.K, b.shape[-1]
    if b.shape[-2] != K:
        raise RuntimeError("gemm_x3_splitk: inner dimensions differ")
    squeeze = b.dim() == 2
    if out is None:
        out = torch.empty((batch, M, N), device=b.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or out.stride(-1) != 1 or tuple(out.shape) != (batch, M, N) or not out.is_cuda:
        raise RuntimeError("gemm_x3_splitk: out must be a (batch, M, N) float32 GPU tensor")
    per, nz, rr, _ = gemm_x3_splitk_plan(M, N, K, batch) if plan is None else (tuple(plan) + (0,))
    need = batch * nz * M * round_up(N, 32)
    ws = _SPLITK_WS.get(b.device)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1 << 22), device=b.device, dtype=torch.float32)
        _SPLITK_WS[b.device] = ws
    q = _gemm_args("gemm_x3_splitk", a.buf, b, out, M, N, K, batch, bias, act, slope, res, k_scale)
    q.lda, q.ldb = K, b.stride(-2)
    q.stride_a, q.stride_b = 0, (b.stride(0) if b.dim() == 3 else 0)
    q.tile_hint, q.pre = 0, (GEMM_PRE_F16X2 if a.split == "f16x2" else 1)
    if _PROFILING:
        set_tag("%dx%dx%d b%d z%d%s" % (M, N, K, batch, nz, " f16x2" if a.split == "f16x2" else ""))
    _check(load().occd_gemm_f32x3_splitk(ctypes.byref(q), per, nz, rr, ws.data_ptr(), ws.numel(), _stream()),
           "occd_gemm_f32x3_splitk")
    return out[0] if squeeze else out


def gemm_x3_nt(a, b, tile_hint=0, splits=None, reduce=True, plain_bf16=False):
    """K16t (occd_gemm_f32x3_nt): a[i] @ b[i].T for a (batch, M, K), b (batch, N, K) -- both k-contiguous, any alignment /
    K: the weight gradient of a pointwise convolution (gy (Cout, HW) x (Cin, HW)).  The reduction dimension is split over
    `splits` workgroup groups (default: the library's proposal); reduce=True returns the (M, N) sum over batch and splits
    (what a weight gradient is), reduce=False the (batch, splits, M, N) partial products."""
    for t, nm in ((a, "a"), (b, "b")):
        if t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda or t.stride(-1) != 1:
            raise RuntimeError(f"gemm_x3_nt: {nm} must be a (batch, rows, K) float32 GPU tensor with unit innermost stride")
    batch, M, K = a.shape
    if b.shape[0] != batch or b.shape[2] != K:
        raise RuntimeError("gemm_x3_nt: operand shapes do not match")
    N = b.shape[1]
    if splits is None:
        splits = load().occd_gemm_f32x3_nt_splits(M, N, K, batch)
    steps = (K + 31) // 32
    per = (steps + splits - 1) // splits
    splits = (steps + per - 1) // per                 # every split owns at least one K step
    out = torch.empty((batch, splits, M, N), device=a.device, dtype=torch.float32)
    q = GemmArgs()
    q.A, q.B, q.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    q.M, q.N, q.K, q.batch = M, N, K, batch
    q.lda, q.ldb, q.ldc = a.stride(1), b.stride(1), N
    q.stride_a, q.stride_b, q.stride_c = a.stride(0), b.stride(0), M * N
    q.tile_hint, q.act, q.pre = tile_hint, splits, (3 if plain_bf16 else 0)
    if _PROFILING:
        set_tag("%dx%dx%d b%d z%d" % (M, N, K, batch, splits))
    _check(load().occd_gemm_f32x3_nt(ctypes.byref(q), _stream()), "occd_gemm_f32x3_nt")
    return out.sum((0, 1)) if reduce else out


class _PwConvFn(torch.autograd.Function):
    """Training: a pointwise (1x1, stride 1, no bias) convolution of an NCHW tensor on K16 / K16t -- forward W . x, data
    gradient W^T . gy (both the NN kernel, float32-level accuracy on the bf16 matrix pipe) and weight gradient gy . x^T (the
    NT kernel, on the tensors as they lie) -- instead of MIOpen / rocBLAS behind `aten::convolution_backward`: the 55 MBConv
    blocks' expand / project convolutions were 13 ms of the 106 ms bf16-mode step (profiles/r04_train_step_bf16_aten_ops.txt)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w):
        from . import autograd3d
        B, C, H, W = x.shape
        xc = x if x.is_contiguous() else x.contiguous()
        ctx.save_for_backward(xc, w)
        ctx.plain = bool(autograd3d.BF16_MFMA) and PW_TRAIN == "bf16"      # (opt-in) one bf16 product instead of the 3-way split
        return gemm_x3(w.detach().reshape(w.shape[0], C), xc.view(B, C, H * W), plain_bf16=ctx.plain).view(B, w.shape[0], H, W)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        B, C, H, W = x.shape
        Co = w.shape[0]
        g = gy.float()
        g = (g if g.is_contiguous() else g.contiguous()).view(B, Co, H * W)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = gemm_x3(w.detach().reshape(Co, C).t().contiguous(), g, plain_bf16=ctx.plain).view(B, C, H, W)
        if ctx.needs_input_grad[1]:
            gw = gemm_x3_nt(g, x.view(B, C, H * W), plain_bf16=ctx.plain).view(Co, C, 1, 1)
        return gx, gw


# OCCDEPTH_TRAIN_PW_GEMM: 1 (default since round 5) = the encoder's pointwise (expand / project) convolutions run forward, data
# gradient and weight gradient on K16 / K16t with the 3-way split (float32-accurate) in training -- the same time as MIOpen /
# rocBLAS on these small shapes (round 4: 153.1 vs 152 ms fp32, 107.7 vs 106.5 ms bf16 mode; round 5: 104.1 / 105.0 vs 104.6 /
# 105.6 ms), but ~13 ms of library work (the largest non-repo share of the step) becomes in-repo and deterministic, and the full
# training-step parity test holds unchanged; 0 = ATen (A/B); bf16 = plain bf16 operands in the bf16-MFMA mode (105.5 vs 106.7 ms)
# -- NOT the default: through the 55 MBConv blocks of a random-init B7 the bf16 rounding of 110 chained pointwise convolutions
# turns the encoder's gradient directions to cosine 0.2 - 0.35 against the real reference (0.93 - 0.97 with the encoder in
# fp32; tests/test_train_step.py::test_train_step_full_config2_matches_reference_gpu).
PW_TRAIN = os.environ.get("OCCDEPTH_TRAIN_PW_GEMM", "1")


def pw_conv_autograd_ok(conv, x):
    """The pointwise convolutions `_PwConvFn` takes: 1x1, stride 1, one group, no bias, channel counts K16 accepts."""
    if PW_TRAIN not in ("1", "bf16"):
        return False
    # float32 inputs only, except under autocast (where _PwConvFn casts): a plain half-precision input falls back to ATen
    # instead of reaching gemm_x3 with operands it rejects
    dt_ok = x.dtype == torch.float32 or (torch.is_autocast_enabled() and x.dtype in (torch.bfloat16, torch.float16))
    return (GEMM_X3 and x.is_cuda and x.dim() == 4 and dt_ok
            and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.groups == 1 and conv.bias is None
            and conv.dilation == (1, 1) and conv.in_channels % 8 == 0 and conv.out_channels % 8 == 0
            and x.shape[2] * x.shape[3] >= 4 and x.shape[0] <= 65535)


def pw_conv_autograd(x, w):
    return _PwConvFn.apply(x, w)


# K16 instead of the library GEMMs in the eval path of the 2-D network (tap GEMMs, Winograd-domain products, expand 1x1
# convolutions, the merged conv_head o conv2).  OCCDEPTH_GEMM_X3=0 restores torch.matmul / torch.bmm / F.conv2d for A/B.
GEMM_X3 = os.environ.get("OCCDEPTH_GEMM_X3", "1") == "1"


# static operands pre-split once (GemmPacked) instead of split on the fly: measured NO gain (tap GEMMs +-3 %, Winograd domain
# 122 against 140 TF/s, frame 21.77 against 21.48 ms; profiles/r04_gemm_x3_v2_presplit.txt) -- the fragment stream from L2 costs
# what the split arithmetic saved -- so it stays an option (tested), off by default
GEMM_X3_PACK = os.environ.get("OCCDEPTH_GEMM_X3_PACK", "0") == "1"


# K16p (round 5): the SHORT-K left operands (expand convolutions, the 1/1 and 1/2 tap GEMMs: K <= 848, >= 256 rows) ARE pre-split, for
# the panel-stationary kernel that keeps a 64-column panel of B over the whole K in LDS (csrc/gemm_x3.hip).  OCCDEPTH_GEMM_X3_PANEL=0
# -> the barrier-phased K16 on float32 operands as in round 4.  Whether a launch takes K16p is the library's own answer
# (`gemm_x3_route`: K <= 352, or K <= 848 on a few-pixel launch); matrices below PANEL_MIN_ROWS rows never do (one row tile for
# each of the 8 waves).
GEMM_X3_PANEL = os.environ.get("OCCDEPTH_GEMM_X3_PANEL", "1") == "1"
PANEL_MIN_ROWS = 256


# K16 on the pre-split weight image (PRE = 1, fragments requested a full 32-k step ahead since late round 5): the long-K
# GEMMs that fill the chip with 256 x 128 tiles -- the tap GEMMs of the 1/4, 1/8 and 1/16 levels: 425 -> 368, 397 -> 355, 438 ->
# 422 us against float32 operands (profiles/r05_gemm_panel.txt); small launches and the Winograd-domain products do not gain.
PRESPLIT_MIN_K, PRESPLIT_MIN_WORKGROUPS = 512, 320


def presplit_wins(M, N, K, batch):
    """The host rule of K16's pre-split form: does the weight image beat float32 operands split on the fly on this launch?"""
    return K >= PRESPLIT_MIN_K and -(-M // 256) * -(-N // 128) * batch >= PRESPLIT_MIN_WORKGROUPS


def gemm_split():
    """'f16x2' / 'bf16x3': which image a `GemmWeights(..., split="switch")` packs for the launches that read pre-split weights
    (K16p, K21, K16's pre-split form) -- OCCDEPTH_GEMM_SPLIT, or the last `set_gemm_split` (the switch is declared in fused.py)."""
    from . import fused
    return fused.GEMM_SPLIT


def set_gemm_split(v):
    """'f16x2' / 'bf16x3'; read at every launch (`gemm_route`): the next one packs the other image if it has none yet."""
    from . import fused
    fused.set_gemm_split(v)


# K21 on the f16x2 image, per launch geometry (tools/bench_gemm_split.py, profiles/gemm_f16x2_ab.txt): 1.19 - 1.27x wherever a
# workgroup has >= 210 (row tile, 16-k step) pairs to multiply, 1.05x at 150 (160 x 1848 x 960: 5 tiles x 30 steps) and 1.00x at
# 126 (384 x 468 x 1344: 6 x 21) -- a launch that small is its panel staging, the second launch and dispatch, whichever split
# multiplies.  Below this many pairs per workgroup a K21 launch keeps the bf16x3 image.
SPLITK_F16X2_MIN_TILE_STEPS = 140


def splitk_f16x2_wins(M, N, K, batch):
    """The host rule of K21: does the f16x2 image beat bf16x3 on this launch under the library's plan?"""
    per, _, rr, _ = gemm_x3_splitk_plan(M, N, K, batch)
    return -(-(-(-M // 32)) // rr) * per >= SPLITK_F16X2_MIN_TILE_STEPS


# K16's tile variants on the f16x2 image below PANEL_MIN_ROWS rows, per launch geometry (tools/bench_gemm_rest.py,
# profiles/gemm_f16x2_rest_ab.txt, replayed graphs, spreads <= 3 %): every such launch of the config-2 frame wins under the
# library's own hint-0 pick -- project convolutions with gate and skip 48 x 28365 x 288 1.30x and 80 x 7191 x 480 1.29x, the first
# projects of a stage 48 x 28365 x 192 1.28x, 80 x 7191 x 288 1.40x, 160 x 1848 x 480 1.61x, the expand 192 x 112850 x 32 1.21x
# (batch 2 each; forcing a variant gains nothing beyond the spread: hint 4 within 2 % of hint 0 where it leads).  The rule covers
# what was measured: 48 ... 255 rows on at least 3000 columns over the batch; anything else keeps float32 operands.
# OCCDEPTH_GEMM_TILE_F16X2=0 -> float32 operands on all of them for A/B.
TILE_F16X2 = os.environ.get("OCCDEPTH_GEMM_TILE_F16X2", "1") == "1"
TILE_F16X2_MIN_ROWS, TILE_F16X2_MIN_COLS = 48, 3000


def tile_f16x2_wins(M, N, K, batch):
    """The host rule of K16's tile variants on the f16x2 image for matrices below PANEL_MIN_ROWS rows (project convolutions with
    their gate and skip, the 192-row expand): does the image beat float32 operands split on the fly on this launch?"""
    return TILE_F16X2 and M >= TILE_F16X2_MIN_ROWS and N * batch >= TILE_F16X2_MIN_COLS


GEMM_KERNELS = {abi.CONSTANTS["OCCD_GEMM_KERNEL_" + n.upper()]: n for n in ("tile", "panel", "ws", "ksplit")}


def gemm_x3_route(M, N, K, batch, pre=0, plain=True, tile_hint=0):
    """(kernel, variant) occd_gemm_f32x3 launches on this problem -- 'panel' (variant: the panel width in 32-column units),
    'tile' / 'ws' / 'ksplit' (variant: 0 .. 4 = 256 x 128, 128 x 128, 128 x 64, 64 x 64, 64 x 256) -- or None where it refuses.
    The library's own rule (occd_gemm_f32x3_route: the function the launch itself follows); host code, no GPU needed."""
    kernel, variant = c_int32(), c_int32()
    if load().occd_gemm_f32x3_route(M, N, K, batch, pre, 1 if plain else 0, tile_hint, ctypes.byref(kernel), ctypes.byref(variant)):
        return None
    return GEMM_KERNELS[kernel.value], variant.value


class GemmWeights:
    """A static operand (weights) of the 2-D network's GEMMs: the folded float32 matrix `w` (role "a": (M, K) / (batch, M, K);
    role "b": (K, N) / (batch, K, N)) and the images of it that launches have asked for, each packed the first time a launch
    routes to it (`gemm_route`): "bf16x3" / "f16x2" (`GemmPacked`) and "k11" (`pw_pack_weights`, role "a").
    split: which image the pre-split routes read -- None = the three-term bf16 image whatever the switch says (explicit callers),
    "switch" = `gemm_split()` at every launch (the model's builders), or a fixed "bf16x3" / "f16x2".
    small: a matrix below PANEL_MIN_ROWS rows may take K16's tile variants on its f16x2 image (`tile_f16x2_wins`).
    A matrix the f16x2 pack refuses (a non-finite weight) remembers that: `image("f16x2")` is None from then on."""

    def __init__(self, w, role, split=None, small=False):
        if role not in ("a", "b") or split not in (None, "switch", "bf16x3", "f16x2"):
            raise RuntimeError("GemmWeights: role 'a' or 'b'; split None, 'switch', 'bf16x3' or 'f16x2'")
        self.w = w.detach().float().contiguous()
        self.role, self.split, self.small = role, split, small
        self.images, self.kernels = {}, {}

    @property
    def shape(self):
        return self.w.shape

    @property
    def is_cuda(self):
        return self.w.is_cuda

    def dim(self):
        return self.w.dim()

    def split_now(self):
        return gemm_split() if self.split == "switch" else (self.split or "bf16x3")

    def image(self, kind):
        if kind not in self.images:
            if kind == "k11":
                self.images[kind] = pw_pack_weights(self.w)
            elif kind == "f16x2":
                try:
                    self.images[kind] = GemmPacked(self.w, self.role, split="f16x2")
                except ValueError:
                    self.images[kind] = None
            else:
                self.images[kind] = GemmPacked(self.w, self.role)
        return self.images[kind]


def _library_kernel(holder, *query):
    """`gemm_x3_route(*query)`, asked once per (M, N, K, batch, pre, plain) and held on the launch's static operand (the library's
    rule reads the shapes and its own process-wide environment only, none of the switches of this module): asked at every
    launch it cost the eager frame 0.06 - 0.09 ms of 14.02, three times the parent's run-to-run spread."""
    memo = getattr(holder, "kernels", None)
    if memo is None:
        return gemm_x3_route(*query)
    if query not in memo:
        memo[query] = gemm_x3_route(*query)
    return memo[query]


# entry: "lib" (torch.matmul + tensor ops), "k16" (gemm_x3), "k21" (gemm_x3_splitk) or "k11" (conv1x1: the caller's, NCHW);
# a / b: the form of each operand, "f32" / "bf16x3" / "f16x2"; kernel: for "k16" the library's (kernel, variant), else None
GemmRoute = collections.namedtuple("GemmRoute", "entry a b kernel")


def gemm_route(M, N, K, batch, a=None, b=None, res=False, k_scale=False, supported=True, project=None, cuda=True):
    """The ONE decision of an eval-path 2-D GEMM launch act(a @ (b * k_scale) + bias) + res: entry point and operand forms, from
    the shapes, the epilogue, the static operands' properties (a / b: `GemmWeights` or None for a plain tensor; nothing is
    packed here), `supported` (`gemm_x3_supported` on the float32 operands) and the switches as they stand now.  Nothing is
    memoised but the library's answer (`_library_kernel`).  project: (k21, k16) for an MBConv project convolution on dense
    operands (y, gate, skip contiguous) -- what the site's measured limits (efficientnet.PW_PROJECT_*) admit on this map; the
    route is K21, K16 or the caller's K11."""
    split = a.split_now() if a is not None else None
    if project:
        k21, k16 = project
        if k21 and GEMM_X3 and cuda and K % 8 == 0 and N >= 4:
            return GemmRoute("k21", split if split == "bf16x3" or splitk_f16x2_wins(M, N, K, batch) else "bf16x3", "f32", None)
        if not (k16 and GEMM_X3 and K % 8 == 0):
            return GemmRoute("k11", "f32", "f32", None)
    if not GEMM_X3 or not supported:
        return GemmRoute("lib", "f32", "f32", None)
    fa = fb = "f32"
    kernel = None
    plain = not res and not k_scale
    if b is not None and b.is_cuda and GEMM_X3_PACK and not k_scale:
        fb = "bf16x3"
    if a is not None and a.is_cuda:
        if GEMM_X3_PACK:
            fa = split
            if fb != "f32":
                fa = fb = "f32"                                          # (K16 reads ONE image: two static operands stay float32)
        elif GEMM_X3_PANEL and a.dim() == 2 and M >= PANEL_MIN_ROWS:
            # (a panel-only image serves the plain epilogue; with a residual / a k scale the float32 operand goes to K16)
            if plain:
                kernel = _library_kernel(a, M, N, K, batch, GEMM_PRE_F16X2 if split == "f16x2" else 1, True)
                if (kernel is not None and kernel[0] == "panel") or presplit_wins(M, N, K, batch):
                    fa = split
                else:
                    kernel = None
        elif GEMM_X3_PANEL and a.dim() == 2 and a.small and split == "f16x2" and tile_f16x2_wins(M, N, K, batch):
            fa = "f16x2"                                                 # K16's tile variants on the image, residual / k scale included
    if kernel is None:
        pre = (GEMM_PRE_F16X2 if fa == "f16x2" else 1) if fa != "f32" else 2 if fb != "f32" else 0
        kernel = _library_kernel(a if a is not None else b, M, N, K, batch, pre, plain)
    return GemmRoute("k16", fa, fb, kernel)


# Rows of a K16 result that start on 128-byte boundaries are WRITTEN 2.2x faster than rows of an odd pixel count (H * W floats:
# every 128-byte store segment straddles two cache lines that another workgroup completes later; tools/store_pattern.hip:
# 650 MB in 121 us against 262 - 290 us; profiles/r05_store_alignment.txt).  `padded_rows` hands out such a result buffer:
# (..., rows, n) as a view of (..., rows, n rounded up to 32 floats).  OCCDEPTH_PAD_ROWS=0 -> dense results as in round 4.
PAD_ROWS = os.environ.get("OCCDEPTH_PAD_ROWS", "1") == "1"


def padded_rows(shape, device):
    """An uninitialised float32 tensor of `shape` whose rows (last dimension) lie 128-byte aligned: a view of a buffer with the
    last dimension rounded up to 32 floats (stride(-1) == 1; the leading dimensions dense over the padded rows)."""
    n = int(shape[-1])
    pitch = round_up(n, 32) if PAD_ROWS else n
    return torch.empty(tuple(shape[:-1]) + (pitch,), device=device, dtype=torch.float32)[..., :n]


def matmul(a, b, bias=None, act=None, slope=0.01, res=None, k_scale=None, out=None, route=None):
    """act(a @ (b * k_scale[..., None]) + bias[:, None]) + res for the eval path, on the route `gemm_route` names (route: the
    caller's, if it asked already): K16 / K21 on the operand forms it says, else the library + plain tensor ops.  a / b: tensors,
    or `GemmWeights` for static operands; out: an optional (batch, M, N) result tensor (rows may be padded: `padded_rows`)."""
    wa, wb = (a if isinstance(a, GemmWeights) else None), (b if isinstance(b, GemmWeights) else None)
    ta, tb = (a.w if wa is not None else a), (b.w if wb is not None else b)
    M, K, N = ta.shape[-2], ta.shape[-1], tb.shape[-1]
    if route is None:
        batch = ta.shape[0] if ta.dim() == 3 else tb.shape[0] if tb.dim() == 3 else 1
        route = gemm_route(M, N, K, batch, wa, wb, res is not None, k_scale is not None, GEMM_X3 and gemm_x3_supported(ta, tb))
    if route.entry != "lib":
        xa, xb = ta, (wb.image(route.b) if route.b != "f32" else tb)
        if route.a != "f32":
            xa = wa.image(route.a)
            if xa is None:       # the f16x2 pack refused a non-finite weight: bf16x3 -- float32 on the tile route, which has no other image
                xa = wa.image("bf16x3") if route.entry == "k21" or GEMM_X3_PACK or M >= PANEL_MIN_ROWS else ta
        if route.entry == "k21":
            return gemm_x3_splitk(xa, tb, bias=bias, act=act, slope=slope, res=res, k_scale=k_scale, out=out)
        return gemm_x3(xa, xb, bias=bias, act=act, slope=slope, res=res, k_scale=k_scale, out=out)
    if k_scale is not None:
        tb = tb * k_scale.unsqueeze(-1)
    y = torch.matmul(ta, tb)
    if bias is not None:
        y = y + bias.view(-1, 1)
    if act == "swish":
        y = y * torch.sigmoid(y)
    elif act == "leaky":
        y = torch.nn.functional.leaky_relu(y, slope)
    y = y + res if res is not None else y
    if out is not None:
        out.copy_(y)
        return out
    return y


def c32x3_eligible(x, cout, kernel, out, stride=(1, 1, 1), dilation=(1, 1, 1), padding=(0, 0, 0), res1=None, res2=None,
                   act_in=ACT_NONE, act_out=ACT_NONE, out_pos=None, o_stride=(1, 1, 1), o_off=(0, 0, 0), cin=None,
                   tile_hint=0):
    """True when `conv3d_bf16(..., split3=True)` takes the sliding-window split kernel K2s3 (the host-side mirror of
    `c32_geometry` + the Z / dilation condition of `try_conv3d_c32_slide_x3` in csrc/conv3d_c32p.hip): the full-resolution head convolutions."""
    d = tuple(dilation)
    if tuple(kernel) != (3, 3, 3) or tuple(stride) != (1, 1, 1) or d[0] != d[1] or d[0] != d[2] or not 1 <= d[0] <= 3:
        return False
    if tuple(padding) != d or (out_pos is not None and tuple(out_pos) != tuple(x.dims)) or tuple(o_stride) != (1, 1, 1) or \
            tuple(o_off) != (0, 0, 0):
        return False
    c = x.C if cin is None else cin
    if round_up(c, 8) != 32 or cout > 32 or x.coff + 32 > x.cs or act_in == ACT_SIGMOID or tile_hint != 0:
        return False
    if x.buf.dtype != torch.float32 or x.cs % 4 or x.coff % 4:
        return False
    X, Y, Z = x.dims
    # Z = 32, or (round 5) any multiple of 32: the z-halo form of the kernel (dilation 3 of a Z > 32 volume on six-row y tiles)
    if Z % 32 or tuple(out.dims) != (X, Y, Z):
        return False
    return x.batch * X * ((Y + 7) // 8) * (Z // 32) >= 512 and x.batch * X * Y * Z * x.cs < 2 ** 32


_wgrad_ws = {}


def conv3d_wgrad(x, gy, cin, cout, kernel, stride=(1, 1, 1), dilation=(1, 1, 1), padding=(0, 0, 0)):
    """dW (cout, cin, kx, ky, kz) of a convolution y = conv(x, W) from channels-last x and gy = dL/dy (K8)."""
    a = WgradArgs()
    a.x, a.gy = _f32(x.buf, "x"), _f32(gy.buf, "gy")
    a.batch = x.batch
    a.X, a.Y, a.Z = x.dims
    a.cin, a.x_cs, a.x_coff = cin, x.cs, x.coff
    a.Xo, a.Yo, a.Zo = gy.dims
    a.cout, a.gy_cs, a.gy_coff = cout, gy.cs, gy.coff
    a.kx, a.ky, a.kz = kernel
    a.sx, a.sy, a.sz = stride
    a.dx, a.dy, a.dz = dilation
    a.px, a.py, a.pz = padding
    need = load().occd_conv3d_wgrad_workspace_floats(ctypes.byref(a))
    if need <= 0:
        raise RuntimeError(f"occd_conv3d_wgrad_workspace_floats failed (code {need})")
    dev = x.buf.device
    ws = _wgrad_ws.get(dev)                      # one growing scratch buffer per device (stream-ordered reuse)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
        _wgrad_ws[dev] = ws
    dw = torch.empty((cout, cin) + tuple(kernel), dtype=torch.float32, device=dev)
    a.dw, a.workspace, a.workspace_floats = dw.data_ptr(), ws.data_ptr(), ws.numel()
    if _PROFILING:
        set_tag("%d>%d k%d%d%d s%d%d%d d%d%d%d @%dx%dx%d" % ((cin, cout) + tuple(kernel) + tuple(stride)
                                                              + tuple(dilation) + tuple(x.dims)))
    _check(load().occd_conv3d_wgrad(ctypes.byref(a), _stream()), "occd_conv3d_wgrad")
    return dw


def conv3d_wgrad_bf16(x, gy, cin, cout, kernel, stride=(1, 1, 1), dilation=(1, 1, 1), padding=(0, 0, 0)):
    """K8b: `conv3d_wgrad` on the bf16 matrix pipe (fp32 accumulate, fp32 result); x / gy both float32 or both bfloat16."""
    code = _storage_code(x.buf.dtype)
    ptr = _act_ptr(x.buf.dtype)
    a = WgradArgs()
    a.x, a.gy = ptr(x.buf, "x"), ptr(gy.buf, "gy")
    a.batch = x.batch
    a.X, a.Y, a.Z = x.dims
    a.cin, a.x_cs, a.x_coff = cin, x.cs, x.coff
    a.Xo, a.Yo, a.Zo = gy.dims
    a.cout, a.gy_cs, a.gy_coff = cout, gy.cs, gy.coff
    a.kx, a.ky, a.kz = kernel
    a.sx, a.sy, a.sz = stride
    a.dx, a.dy, a.dz = dilation
    a.px, a.py, a.pz = padding
    need = load().occd_conv3d_wgrad_bf16_workspace_floats(ctypes.byref(a), code)
    if need <= 0:
        raise RuntimeError(f"occd_conv3d_wgrad_bf16_workspace_floats failed (code {need})")
    dev = x.buf.device
    ws = _wgrad_ws.get(dev)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.float32, device=dev)
        _wgrad_ws[dev] = ws
    dw = torch.empty((cout, cin) + tuple(kernel), dtype=torch.float32, device=dev)
    a.dw, a.workspace, a.workspace_floats = dw.data_ptr(), ws.data_ptr(), ws.numel()
    if _PROFILING:
        set_tag("%d>%d k%d%d%d s%d%d%d d%d%d%d @%dx%dx%d" % ((cin, cout) + tuple(kernel) + tuple(stride)
                                                              + tuple(dilation) + tuple(x.dims)))
    _check(load().occd_conv3d_wgrad_bf16(ctypes.byref(a), code, _stream()), "occd_conv3d_wgrad_bf16")
    return dw


# ----------------------------------------------------------------------------- K1
class Frustum:
    """The operands of the FLoSP-Depth frustum sample (occd_flosp_args without its output), so that the sample can run
    either on its own (`flosp_sample`) or inside the fused lift (`lift_proj`)."""

    def __init__(self, depth, trans, proj, ida, voxel_num, final_dim, d_min, d_max, mean_mode=True, grids=None):
        self.depth, self.trans, self.proj, self.ida, self.grids = depth, trans, proj, ida, grids
        self.voxel_num = tuple(int(v) for v in voxel_num)
        self.final_dim, self.d_min, self.d_max, self.mean_mode = final_dim, d_min, d_max, mean_mode

    def fill(self, a):
        B, V, D, h, w = self.depth.shape
        a.depth = _f32(self.depth, "depth")
        if self.grids is None:
            a.trans, a.proj, a.ida = _f32(self.trans, "trans"), _f32(self.proj, "proj"), _f32(self.ida, "ida")
        else:
            a.grids = _f32(self.grids, "grids")
        a.batch, a.n_cams, a.D, a.h, a.w = B, V, D, h, w
        a.A, a.Bdim, a.C = self.voxel_num
        a.img_h, a.img_w = float(self.final_dim[0]), float(self.final_dim[1])
        a.depth_min, a.depth_max = float(self.d_min), float(self.d_max)
        a.mean_mode = 1 if self.mean_mode else 0

    def sample(self):
        B = self.depth.shape[0]
        A, Bd, C = self.voxel_num
        out = torch.empty((B, A * Bd * C), device=self.depth.device, dtype=torch.float32)
        a = FlospArgs()
        self.fill(a)
        a.out = _f32(out, "out")
        _check(load().occd_flosp_sample_fwd(ctypes.byref(a), _stream()), "occd_flosp_sample_fwd")
        return out


def flosp_sample_bwd(fr, gout):
    """d loss / d depth (B, V, D, h, w) of `fr.sample()` given gout (B, A*B*C): the transpose of the frustum sample,
    deterministic (occd_flosp_sample_bwd)."""
    B, V, D, h, w = fr.depth.shape
    gdepth = torch.empty((B, V, D, h, w), device=gout.device, dtype=torch.float32)
    ws = torch.empty(B * V * D * h * w + 1, dtype=torch.int64, device=gout.device)
    q = FlospBwdArgs()
    fr.fill(q.fwd)
    q.gout = _f32(gout, "gout")
    q.gdepth = gdepth.data_ptr()
    q.workspace, q.workspace_bytes = ws.data_ptr(), ws.numel() * 8
    _check(load().occd_flosp_sample_bwd(ctypes.byref(q), _stream()), "occd_flosp_sample_bwd")
    return gdepth


def flosp_sample(depth, trans, proj, ida, voxel_num, final_dim, d_min, d_max, mean_mode=True, grids=None):
    """depth (B, V, D, h, w) -> (B, A*B*C) sampled voxel volume (see occd_flosp_sample_fwd)."""
    return Frustum(depth, trans, proj, ida, voxel_num, final_dim, d_min, d_max, mean_mode, grids).sample()


# workgroup -> XCD placement of the lift (profiles/r02_lift_xcd_modes.txt): 2 = y-blocks per XCD, the HBM fetch of the
# config-2 lift drops from 282 MB (dispatch order) to 174 MB = the distinct bytes
LIFT_XCD_MODE = int(os.environ.get("OCCDEPTH_LIFT_XCD", "2"))


def _lift_args(a, feats, scale_divs, pix, fov, n_dims, row_strides, out, depth_scale, scale_const, xcd_mode):
    S, V = len(feats), len(feats[0])
    B = feats[0][0].shape[0]
    for s in range(S):
        for v in range(V):
            f = feats[s][v]
            if f.dtype != torch.float32 or not f.is_cuda:
                raise RuntimeError("feature rows must be float32 GPU tensors")
            if not f[0].is_contiguous():
                raise RuntimeError("every image of a feature-row tensor must be dense (H, W, cs)")
            a.feat[s][v] = f.data_ptr()
            a.feat_bstride[s][v] = f.stride(0) if f.shape[0] > 1 else 0
        a.feat_h[s], a.feat_w[s] = feats[s][0].shape[1], feats[s][0].shape[2]
        a.feat_cs[s] = feats[s][0].shape[3]
        a.scale_div[s] = int(scale_divs[s])
    a.n_scales, a.n_views, a.batch = S, V, B
    a.C = out.C
    if pix is None:                    # occd_lift_proj_fwd: the kernel projects
        a.N, a.P = int(n_dims[0]) * int(n_dims[1]) * int(n_dims[2]), 1
    else:
        if pix.dtype != torch.int64:
            raise RuntimeError("projected_pix must be int64")
        a.pix = _ptr(pix, "projected_pix")
        fov8 = fov.view(torch.uint8) if fov.dtype == torch.bool else fov
        if fov8.dtype != torch.uint8:
            raise RuntimeError("fov_mask must be bool/uint8")
        a.fov = _ptr(fov8, "fov_mask")
        a.N, a.P = pix.shape[2], pix.shape[3]
    if depth_scale is not None:
        a.depth_scale = _f32(depth_scale, "depth_scale")
    a.scale_const = float(scale_const)
    a.dimA, a.dimB, a.dimC = n_dims
    a.row_a, a.row_b, a.row_c = row_strides
    a.out = _f32(out.buf, "out")
    a.out_rows = out.dims[0] * out.dims[1] * out.dims[2]
    a.out_cs = out.cs
    a.xcd_mode = LIFT_XCD_MODE if xcd_mode is None else int(xcd_mode)
    if out.coff != 0:
        raise RuntimeError("lift output must start at channel 0")


def lift(feats, scale_divs, pix, fov, n_dims, row_strides, out, depth_scale=None, scale_const=100.0, xcd_mode=None):
    """feats[s][v]: (B, H_s, W_s, cs) channels-last maps (dense per image; the batch stride is free); pix (B, V, N, P, 2)
    int64; fov (B, V, N, P) bool.

    Writes out.buf rows (channels-last voxel grid); n -> (a,b,c) over n_dims, row = a*ra + b*rb + c*rc."""
    a = LiftArgs()
    _lift_args(a, feats, scale_divs, pix, fov, n_dims, row_strides, out, depth_scale, scale_const, xcd_mode)
    _check(load().occd_lift_fwd(ctypes.byref(a), _stream()), "occd_lift_fwd")
    return out


class RowsGemmWeights:
    """The fragment-ordered image of a dense (K, N) float32 matrix for `rows_gemm` (occd_rows_gemm_pack)."""

    def __init__(self, w_rows):
        if w_rows.dtype != torch.float32 or w_rows.stride(1) != 1 or not w_rows.is_cuda:
            raise RuntimeError("rows_gemm: the weight matrix must be a float32 GPU tensor with unit column stride")
        self.K, self.N = int(w_rows.shape[0]), int(w_rows.shape[1])
        self.buf = torch.empty(load().occd_rows_gemm_packed_floats(self.K, self.N), device=w_rows.device, dtype=torch.float32)
        _check(load().occd_rows_gemm_pack(w_rows.data_ptr(), self.buf.data_ptr(), self.K, self.N, int(w_rows.stride(0)),
                                          _stream()), "occd_rows_gemm_pack")


def rows_gemm(a, w, out, bias=None, res=None, act_in=ACT_NONE, act_out=ACT_NONE):
    """K15: out[row, :N] = act_out(act_in(a[row, :K]) @ W[:K, :N] + bias (+ res[row, :N])) on float32 Vox rows;
    w: a dense (K, N) float32 device matrix (packed on the fly) or a `RowsGemmWeights`."""
    if not isinstance(w, RowsGemmWeights):
        w = RowsGemmWeights(w)
    K, N = w.K, w.N
    q = RowsGemmArgs()
    q.a, q.w, q.out = _f32(a.buf, "a"), w.buf.data_ptr(), _f32(out.buf, "out")
    q.bias = _f32(bias, "bias") if bias is not None else None
    q.res = _f32(res.buf, "res") if res is not None else None
    q.rows = a.batch * a.dims[0] * a.dims[1] * a.dims[2]
    q.K, q.N = K, N
    q.a_cs, q.a_coff, q.out_cs, q.out_coff = a.cs, a.coff, out.cs, out.coff
    if res is not None:
        q.res_cs, q.res_coff = res.cs, res.coff
    q.w_stride = N
    q.act_in, q.act_out = act_in, act_out
    if _PROFILING:
        set_tag("%d>%d @%d rows" % (K, N, q.rows))
    _check(load().occd_rows_gemm_fwd(ctypes.byref(q), _stream()), "occd_rows_gemm_fwd")
    return out


def rows_gemm_supported(K, N, a, out, res=None):
    """(N % 8: the kernel writes exactly N channels, and the consumers of a Vox read its rows in 8-channel groups)"""
    ok = K % 16 == 0 and N % 8 == 0 and a.cs % 4 == 0 and a.coff % 4 == 0 and out.cs % 4 == 0 and out.coff % 4 == 0
    ok = ok and a.buf.dtype == torch.float32 and a.coff + K <= a.cs and out.coff + N <= out.cs
    return ok and (res is None or (res.cs % 4 == 0 and res.coff % 4 == 0))


def bottleneck3d_supported(C, P, dims):
    """Geometries K14 (occd_bottleneck3d_fwd) is built for; everything else keeps the five-launch K2 form."""
    return P in (16, 32) and C % 16 == 0 and dims[2] in (4, 8, 16)


def bottleneck3d(x, w, P, dilation, out=None):
    """K14: y = one stride-1 DDR Bottleneck3D of the float32 Vox x (BatchNorm folded into `w`, packed as
    occd_bottleneck3d_fwd documents); dilation = (d_z, d_y, d_x) of conv2 / conv3 / conv4."""
    C = x.C
    if w.dtype != torch.float32 or w.numel() != load().occd_bottleneck3d_weight_floats(C, P):
        raise RuntimeError("bottleneck3d: packed weight buffer has the wrong size")
    if out is None:
        out = Vox.empty(x.batch, x.dims, C, x.buf.device)
    X, Y, Z = x.dims
    o2 = torch.empty(x.batch * X * Y * Z * P, device=x.buf.device, dtype=torch.float32)
    a = BneckArgs()
    a.x, a.y, a.o2, a.w = _f32(x.buf, "x"), _f32(out.buf, "y"), _f32(o2, "o2"), _f32(w, "w")
    a.batch, a.X, a.Y, a.Z, a.C, a.P = x.batch, X, Y, Z, C, P
    a.x_cs, a.x_coff, a.y_cs, a.y_coff = x.cs, x.coff, out.cs, out.coff
    a.d0, a.d1, a.d2 = (int(d) for d in dilation)
    if _PROFILING:
        set_tag("%d/%d d%d%d%d @%dx%dx%d" % ((C, P) + tuple(int(d) for d in dilation) + (X, Y, Z)))
    _check(load().occd_bottleneck3d_fwd(ctypes.byref(a), _stream()), "occd_bottleneck3d_fwd")
    return out


def _check_calibration(B, V, cam_E, cam_k, ida=None):
    for t, shape, what, dt in ((cam_E, (4, 4), "cam_E", torch.float64), (cam_k, (3, 3), "cam_k", torch.float64),
                               (ida, (4, 4), "ida", torch.float32)):
        if t is None and what == "ida":
            continue
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (B, V) + shape:
            raise RuntimeError(f"{what} must be a contiguous (batch, views, {shape[0]}, {shape[1]}) {dt} GPU tensor")


def lift_proj(feats, scale_divs, cam_E, cam_k, origin, voxel_size, img_wh, n_dims, row_strides, out, frustum=None,
              scale_const=100.0, xcd_mode=None, ida=None):
    """The eval lift without its tables (occd_lift_proj_fwd): cam_E (B, V, 4, 4) / cam_k (B, V, 3, 3) float64 device
    tensors (the batch's extrinsics and intrinsics), the voxel grid n_dims = (X, Y, Z) of `voxel_size` metres from
    `origin`; frustum: a `Frustum` or None; ida: the batch's (B, V, 4, 4) float32 device ida_mats or None -- a view with
    ida[b, v, 0, 0] < 0 gathers its in-FOV pixels at x' = W - 1 - x (the reference's left-right flip)."""
    q = LiftProjArgs()
    _lift_args(q.lift, feats, scale_divs, None, None, n_dims, row_strides, out, None, scale_const, xcd_mode)
    _check_calibration(q.lift.batch, q.lift.n_views, cam_E, cam_k, ida)
    q.cam_E, q.cam_k = cam_E.data_ptr(), cam_k.data_ptr()
    q.ida = ida.data_ptr() if ida is not None else None
    q.voxel_size = float(voxel_size)
    for j in range(3):
        q.origin[j] = float(origin[j])
    q.img_w, q.img_h = int(img_wh[0]), int(img_wh[1])
    if frustum is not None:
        frustum.fill(q.frustum)
    if _PROFILING:
        set_tag("%d scales x %d views x %d ch > %d voxels" % (q.lift.n_scales, q.lift.n_views, q.lift.C, q.lift.N))
    _check(load().occd_lift_proj_fwd(ctypes.byref(q), _stream()), "occd_lift_proj_fwd")
    return out


def lift_backward(feats, scale_divs, pix, fov, n_dims, row_strides, out_like, gout, depth_scale=None, scale_const=100.0):
    """Backward of `lift` (single-point patterns): gout (B, X, Y, Z, cs) channels-last d loss / d out ->
    ([[d loss / d feats[s][v] (same shape, channels-last rows)]], d loss / d depth_scale (B, N) or None)."""
    q = LiftBwdArgs()
    _lift_args(q.fwd, feats, scale_divs, pix, fov, n_dims, row_strides, out_like, depth_scale, scale_const, 0)
    q.gout = _f32(gout, "gout")
    grads = []
    for s, per_scale in enumerate(feats):
        row = []
        for v, f in enumerate(per_scale):
            g = torch.zeros_like(f)
            if g.stride() != f.stride():
                raise RuntimeError("gradient map layout differs from the feature map's")
            q.gfeat[s][v] = g.data_ptr()
            row.append(g)
        grads.append(row)
    gd = None
    if depth_scale is not None:
        gd = torch.empty_like(depth_scale)
        q.gdepth = gd.data_ptr()
    _check(load().occd_lift_bwd(ctypes.byref(q), _stream()), "occd_lift_bwd")
    return grads, gd


# ----------------------------------------------------------------------------- helpers
def nchw_to_nhwc(x, cs=None):
    """(B, C, *spatial) -> (B, *spatial, cs) channels-last copy with zero pad."""
    B, C = x.shape[0], x.shape[1]
    sp = tuple(x.shape[2:])
    S = 1
    for d in sp:
        S *= d
    cs = cs if cs is not None else round_up(C, 4)
    out = torch.empty((B,) + sp + (cs,), device=x.device, dtype=torch.float32)
    xc = x.contiguous()
    _check(load().occd_nchw_to_nhwc(_f32(xc, "x"), _f32(out, "out"), B, C, S, cs, _stream()), "occd_nchw_to_nhwc")
    return out


def nhwc_to_nchw(vox):
    """Vox -> dense (B, C, X, Y, Z) tensor (a real copy; Vox.ncdhw() is the zero-copy view)."""
    B = vox.batch
    X, Y, Z = vox.dims
    out = torch.empty((B, vox.C, X, Y, Z), device=vox.buf.device, dtype=torch.float32)
    _check(load().occd_nhwc_to_nchw(_f32(vox.buf, "in"), _f32(out, "out"), B, vox.C, X * Y * Z, vox.cs, vox.coff,
                                    _stream()), "occd_nhwc_to_nchw")
    return out


def softmax_channels(src, dst, n, dst_pad=0):
    """softmax over src's n logical channels -> dst's n logical channels (+ dst_pad zeros) on the same grid."""
    rows = src.batch * src.dims[0] * src.dims[1] * src.dims[2]
    if _PROFILING:
        set_tag("%d @%d rows" % (n, rows))
    _check(load().occd_softmax_channels(_f32(src.buf, "src"), _f32(dst.buf, "dst"), rows, src.cs, src.coff, dst.cs,
                                        dst.coff, n, dst_pad, _stream()), "occd_softmax_channels")
    return dst


# ----------------------------------------------------------------------------- 2-D NCHW helpers
ACT2D = {None: 0, "none": 0, "relu": 1, "swish": 2, "leaky": 3}


def affine_act(x, scale, shift, act=None, slope=0.01, res=None, res_first=False, out=None):
    """y = act(x * scale[c] + shift[c]) (+ res) on (B, C, *spatial) float32; in place unless `out` is given."""
    if not x.is_contiguous():
        x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    S = x.numel() // (B * C)
    out = x if out is None else out
    if res is not None and not res.is_contiguous():
        res = res.contiguous()
    if _PROFILING:
        set_tag("%d @%dx%d" % (C, B, S))
    _check(load().occd_affine_act_nchw(_f32(x, "x"), _f32(res, "res") if res is not None else None, _f32(out, "out"),
                                       _f32(scale, "scale") if scale is not None else None,
                                       _f32(shift, "shift") if shift is not None else None, B, C, S, ACT2D[act],
                                       float(slope), 1 if res_first else 0, _stream()), "occd_affine_act_nchw")
    return out


_WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def winograd_weights(w):
    """(Cout, Cin, 3, 3) -> U (16, Cin, Cout) with U[4i+j][ci][co] = (G g G^T)[i][j] (float64 arithmetic, once per weight)."""
    G = torch.tensor(_WINO_G, dtype=torch.float64, device=w.device)
    u = torch.einsum("ia,ocab,jb->ijco", G, w.detach().double(), G)
    return u.reshape(16, w.shape[1], w.shape[0]).float().contiguous()


def wino_input_transform(x, ty0=0, ths=None):
    """x (B, C, H, W) -> V (16, B * ths * tw, C) for the tile rows [ty0, ty0 + ths) (default: all)."""
    B, C, H, W = x.shape
    ths = (H + 1) // 2 - ty0 if ths is None else ths
    T = B * ths * ((W + 1) // 2)
    V = torch.empty((16, T, C), device=x.device, dtype=torch.float32)
    xc = x if x.is_contiguous() else x.contiguous()
    if _PROFILING:
        set_tag("%d @%dx%dx%d" % (C, B, H, W))
    _check(load().occd_wino_input_transform_nchw(_f32(xc, "x"), V.data_ptr(), B, C, H, W, ty0, ths, _stream()),
           "occd_wino_input_transform_nchw")
    return V


def wino_output_transform(M, shape, scale=None, shift=None, act=None, slope=0.01, res=None, res_first=False, out=None,
                          ty0=0, ths=None):
    """M (16, B * ths * tw, C) -> rows [2 ty0, 2 (ty0 + ths)) of y (B, C, H, W) (allocated unless `out` is given)."""
    B, C, H, W = shape
    ths = (H + 1) // 2 - ty0 if ths is None else ths
    y = torch.empty(shape, device=M.device, dtype=torch.float32) if out is None else out
    if res is not None and not res.is_contiguous():
        res = res.contiguous()
    if _PROFILING:
        set_tag("%d @%dx%dx%d" % (C, B, H, W))
    _check(load().occd_wino_output_transform_nchw(_f32(M, "M"), _f32(scale, "scale") if scale is not None else None,
                                                  _f32(shift, "shift") if shift is not None else None,
                                                  _f32(res, "res") if res is not None else None, _f32(y, "y"), B, C, H, W,
                                                  ty0, ths, ACT2D[act], float(slope), 1 if res_first else 0, _stream()),
           "occd_wino_output_transform_nchw")
    return y


class WinoCM:
    """The weight operand of the channel-major Winograd-domain product: U^T (16, Cout, Cin) as the batch-16 f16x2 image of
    `GemmPacked(..., "a", split="f16x2")`.  `make_u` builds the operand of the present form (`GemmWeights(U, "b")`)
    the first time a launch needs it (a geometry `wino_cm_wins` turns down, the strip mode): the 16 * Cin * Cout float32 U does
    not stay alive beside the image otherwise.  Raises ValueError on a non-finite weight (no f16x2 image)."""

    def __init__(self, w, make_u):
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        ut = winograd_weights(w).transpose(1, 2).contiguous()             # (16, Cout, Cin)
        self.image = GemmPacked(ut, "a", split="f16x2")
        self._make_u, self._u = make_u, None

    def u(self):
        if self._u is None:
            self._u = self._make_u()
        return self._u


# The channel-major form per launch geometry (tools/bench_gemm_rest.py, profiles/gemm_f16x2_rest_ab.txt; replayed graphs, ms):
#   1280 -> 1280 @2x24x77  (T =  936): whole convolution 0.407 -> 0.245 (1.66x); product 0.333 -> 0.194 (147 -> 253 TF/s)
#    640 ->  640 @2x47x153 (T = 3696): whole convolution 0.421 -> 0.314 (1.34x); product 0.313 -> 0.221 (155 -> 219 TF/s)
# the input transforms 1.72x / 1.47x, the output transforms 1.43x / 1.25x; spreads <= 7 %.  Both are long-K launches that fill
# the chip with 256 x 128 tiles -- the regime in which K16's pre-split form leads on the tap GEMMs (`presplit_wins`, the same
# two limits).  Anything smaller is unmeasured and stays on the present form.  OCCDEPTH_WINO_CM=0 -> the present form for A/B.
WINO_CM = os.environ.get("OCCDEPTH_WINO_CM", "1") == "1"
WINO_CM_MIN_CIN, WINO_CM_MIN_WORKGROUPS = 512, 320


def wino_cm_wins(B, cin, cout, H, W):
    """The host rule of the channel-major Winograd-domain product: does transforms_cm + K16 on the f16x2 image of U^T beat the
    present transforms + K16 on float32 operands on this launch?"""
    T = B * ((H + 1) // 2) * ((W + 1) // 2)
    return WINO_CM and cin >= WINO_CM_MIN_CIN and cin % 8 == 0 and T >= 4 and \
        16 * -(-cout // 256) * -(-T // 128) >= WINO_CM_MIN_WORKGROUPS


def wino_input_transform_cm(x, Tp=None):
    """x (B, C, H, W) -> V^T (16, C, T) as a view of (16, C, Tp), Tp = T rounded up to 32 floats (columns [T, Tp) unwritten)."""
    B, C, H, W = x.shape
    T = B * ((H + 1) // 2) * ((W + 1) // 2)
    Tp = round_up(T, 32) if Tp is None else Tp
    Vt = torch.empty((16, C, Tp), device=x.device, dtype=torch.float32)
    xc = x if x.is_contiguous() else x.contiguous()
    if _PROFILING:
        set_tag("%d @%dx%dx%d" % (C, B, H, W))
    _check(load().occd_wino_input_transform_cm(_f32(xc, "x"), Vt.data_ptr(), B, C, H, W, Tp, _stream()),
           "occd_wino_input_transform_cm")
    return Vt[..., :T]


def wino_output_transform_cm(Mt, shape, scale=None, shift=None, act=None, slope=0.01, res=None, res_first=False):
    """M^T (16, C, T) with rows on a pitch of Tp = Mt.stride(1) floats (Tp % 32 == 0) -> y (B, C, H, W)."""
    B, C, H, W = shape
    T = B * ((H + 1) // 2) * ((W + 1) // 2)
    if Mt.dtype != torch.float32 or tuple(Mt.shape) != (16, C, T) or Mt.stride(2) != 1 or Mt.stride(0) != C * Mt.stride(1):
        raise RuntimeError("wino_output_transform_cm: M^T must be (16, C, T) float32 over dense padded rows")
    y = torch.empty(shape, device=Mt.device, dtype=torch.float32)
    if res is not None and not res.is_contiguous():
        res = res.contiguous()
    if _PROFILING:
        set_tag("%d @%dx%dx%d" % (C, B, H, W))
    if not Mt.is_cuda or Mt.stride(1) < T or Mt.stride(1) % 32:
        raise RuntimeError("wino_output_transform_cm: M^T must be a GPU tensor with rows on a pitch of 32 floats")
    _check(load().occd_wino_output_transform_cm(Mt.data_ptr(), _f32(scale, "scale") if scale is not None else None,
                                                _f32(shift, "shift") if shift is not None else None,
                                                _f32(res, "res") if res is not None else None, _f32(y, "y"), B, C, H, W,
                                                Mt.stride(1), ACT2D[act], float(slope), 1 if res_first else 0, _stream()),
           "occd_wino_output_transform_cm")
    return y


def conv2d_3x3_winograd(x, U, scale=None, shift=None, act=None, slope=0.01, res=None, res_first=False, strip_rows=None,
                        cm=None):
    """act(scale * conv3x3(x, g, pad 1) + shift) (+res) with U = winograd_weights(g) (or `GemmWeights(U, "b")`):
    HIP transforms around 16 batched GEMMs (K16; the library with OCCDEPTH_GEMM_X3=0).  `strip_rows` tile rows per pass keep
    V / M cache-sized on big images.
    U a `WinoCM`: the channel-major form -- channel-major transforms around ONE K16 launch on the f16x2 image of U^T (three fp16
    MFMAs per K step; finite |x| >= 8190 overflow the staged fp16 operand, |V| <= 4 max|x|) -- where `wino_cm_wins` says so
    (cm: None = ask the rule, True / False = force) and the whole image is one pass; else the present form on `U.u()`."""
    B, Cin, H, W = x.shape
    th = (H + 1) // 2
    if isinstance(U, WinoCM):
        whole = strip_rows is None or strip_rows >= th
        if GEMM_X3 and whole and x.is_cuda and (wino_cm_wins(B, Cin, U.cout, H, W) if cm is None else cm):
            if U.cin != Cin:
                raise RuntimeError("conv2d_3x3_winograd: the WinoCM operand does not match the input channels")
            Vt = wino_input_transform_cm(x)
            Mt = torch.empty((16, U.cout, Vt.stride(1)), device=x.device, dtype=torch.float32)[..., :Vt.shape[2]]
            gemm_x3(U.image, Vt, out=Mt)
            return wino_output_transform_cm(Mt, (B, U.cout, H, W), scale, shift, act, slope, res, res_first)
        U = U.u()
    cout = U.shape[2]
    if strip_rows is None or strip_rows >= th:
        V = wino_input_transform(x)
        return wino_output_transform(matmul(V, U), (B, cout, H, W), scale, shift, act, slope, res, res_first)
    y = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32)
    xc = x if x.is_contiguous() else x.contiguous()
    for ty0 in range(0, th, strip_rows):
        ths = min(strip_rows, th - ty0)
        M = matmul(wino_input_transform(xc, ty0, ths), U)
        wino_output_transform(M, tuple(y.shape), scale, shift, act, slope, res, res_first, out=y, ty0=ty0, ths=ths)
    return y


def wino_pack_weights(w, scale=None):
    """(Cout, Cin, 3, 3) conv weight (+ per-cout scale, e.g. a folded BatchNorm) -> packed Winograd-domain operand of K10."""
    cout, cin = w.shape[0], w.shape[1]
    if tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("wino_pack_weights needs a (Cout, Cin, 3, 3) weight")
    n = load().occd_wino_packed_floats(cout, cin)
    if n <= 0:
        raise RuntimeError("occd_wino_packed_floats: bad shape")
    wc = w.detach().float().contiguous()
    upk = torch.empty(n, device=w.device, dtype=torch.float32)
    sc = scale.detach().float().contiguous() if scale is not None else None
    _check(load().occd_wino_pack_weights(_f32(wc, "w"), _f32(sc, "scale") if sc is not None else None,
                                         _f32(upk, "upk"), cout, cin, _stream()), "occd_wino_pack_weights")
    return upk


class WinoF16x2:
    """The weight operand of K10h (wino_pack_weights_f16x2): conv2d_3x3_fused takes K10h when it is handed one of these."""

    __slots__ = ("image", "cout", "cin", "f32")

    def __init__(self, image, cout, cin, f32=None):
        # f32: K10's image of the same weights, or None.  With it, the launch geometries K10h does not win stay on K10.
        self.image, self.cout, self.cin, self.f32 = image, cout, cin, f32


_CU_COUNT = {}


def _cu_count(device):
    n = _CU_COUNT.get(device)
    if n is None:
        n = _CU_COUNT[device] = torch.cuda.get_device_properties(device).multi_processor_count
    return n


def wino_f16x2_wins(B, cin, cout, H, W, device=None):
    """Whether a launch takes K10h when its operand carries both images: launches of at least one workgroup (128 tiles x 32
    couts) per CU do.  K10h is 1.14 - 1.39x faster on every geometry of the config-2 frame (tools/bench_wino_split.py,
    profiles/wino_f16x2_ab.txt), the 120-workgroup DepthNet launches included (1.23x, 71 us per frame together); those stay on
    K10 for now -- DESIGN.md, K10h section, says why -- and moving them is the follow-up."""
    tiles = B * ((H + 1) // 2) * ((W + 1) // 2)
    return ((cout + 31) // 32) * ((tiles + 127) // 128) >= _cu_count(torch.cuda.current_device() if device is None else device)


def wino_pack_weights_f16x2(w, scale=None):
    """(Cout, Cin, 3, 3) conv weight (+ per-cout scale) -> WinoF16x2, the operand of K10h: two fp16 images hi | lo of the
    per-channel power-of-two scaled G g G^T scale plus the epilogue factors.  ValueError when a weight (times scale) is not
    finite (the pack reports it; it synchronises the stream)."""
    cout, cin = w.shape[0], w.shape[1]
    if tuple(w.shape[2:]) != (3, 3):
        raise RuntimeError("wino_pack_weights_f16x2 needs a (Cout, Cin, 3, 3) weight")
    n = load().occd_wino_packed_f16x2_bytes(cout, cin)
    if n <= 0:
        raise RuntimeError("occd_wino_packed_f16x2_bytes: bad shape")
    wc = w.detach().float().contiguous()
    sc = scale.detach().float().contiguous() if scale is not None else None
    image = torch.empty(n, device=w.device, dtype=torch.uint8)
    rc = load().occd_wino_pack_weights_f16x2(_f32(wc, "w"), _f32(sc, "scale") if sc is not None else None,
                                             _ptr(image, "upk"), cout, cin, _stream())
    if rc == -1:
        raise ValueError("wino_pack_weights_f16x2: non-finite weights (keep the float32 image of wino_pack_weights)")
    _check(rc, "occd_wino_pack_weights_f16x2")
    return WinoF16x2(image, cout, cin)


def _parse_wino_persist(value):
    if value not in ("0", "1"):
        raise ValueError("OCCDEPTH_WINO_PERSIST must be 0 or 1, not %r" % (value,))
    return value == "1"


# 1: K10h with persistent workgroups (one per CU walks the tiles, the next tile's first patch lands under the epilogue) -- opt-in:
# bit-identical, 1 - 3 % per launch, no gain outside the run-to-run range in the frame; 0 (default): one
# workgroup per tile block, the form the persistent one is checked against bit for bit (tests/test_wino_persist.py)
WINO_PERSIST = _parse_wino_persist(os.environ.get("OCCDEPTH_WINO_PERSIST", "0"))


def _parse_wino_cout_pair(value):
    if value not in ("auto", "0", "1"):
        raise ValueError("OCCDEPTH_WINO_COUT_PAIR must be auto, 0 or 1, not %r" % (value,))
    return None if value == "auto" else value == "1"


# K10h's work item: 1 = the cout-pair form (two blocks of 32 couts share one patch fetch, transform and split; bit-identical,
# tests/test_wino_cout_pair.py) on every K10h launch, 0 = one cout block per item on every launch, auto (default) = the pair
# form where wino_cout_pair_wins says so
WINO_COUT_PAIR = _parse_wino_cout_pair(os.environ.get("OCCDEPTH_WINO_COUT_PAIR", "auto"))

# (cin, cout, H, W) at batch 2 of the config-2 frame's K10h launches whose pair form's WORST round beat the one-block form's
# BEST round in tools/bench_wino_pair.py (profiles/wino_cout_pair_ab.txt).  An exact-geometry table: any other resolution or
# batch size keeps the one-block form unless OCCDEPTH_WINO_COUT_PAIR=1.  (128, 128, 47, 153) and (64, 128, 47, 153) are DepthNet's
# launches, which wino_f16x2_wins keeps on K10: the two entries take effect only where K10h is forced on them.
WINO_COUT_PAIR_TABLE = frozenset({(160, 160, 185, 610), (320, 320, 93, 305), (128, 128, 47, 153), (32, 160, 185, 610),
                                  (48, 320, 93, 305), (224, 1280, 24, 77), (80, 640, 47, 153), (64, 128, 47, 153)})


def wino_cout_pair_wins(B, cin, cout, H, W):
    """Whether a K10h launch takes the cout-pair form by default: only the measured launch geometries of the table above;
    everything else is unmeasured and stays on the one-block form."""
    return B == 2 and (cin, cout, H, W) in WINO_COUT_PAIR_TABLE


def conv2d_3x3_fused(x, upk, cout, shift=None, act=None, slope=0.01, res=None, res_first=False, tile_hint=0, out=None,
                     max_workgroups=None, cout_blocks=None):
    """K10: act(conv3x3(x, g * scale, pad 1) + shift) (+ res) in one launch (upk = wino_pack_weights(g, scale)); K10h, the
    same on the two-term fp16 split, when upk is the WinoF16x2 of wino_pack_weights_f16x2(g, scale).  max_workgroups (K10h
    only; RuntimeError with a K10 operand; without effect on a launch that wino_f16x2_wins sends to the K10 image of a WinoF16x2):
    0 = persistent workgroups, one per CU (the one-item form when the launch has no more items than that); k > 0 = at most k
    persistent workgroups; -1 = one workgroup per tile block; None = WINO_PERSIST's choice between 0 and -1.  cout_blocks (K10h
    only): 1 = one block of 32 couts per work item; 2 = the cout-pair form, which has one workgroup per item only (it takes
    max_workgroups None as -1 and refuses max_workgroups >= 0); None = WINO_COUT_PAIR's choice (auto: wino_cout_pair_wins),
    where a persistent grid, asked for by max_workgroups or by WINO_PERSIST, keeps the one-block form.  Same bits either way."""
    if not x.is_contiguous():
        x = x.contiguous()
    B, cin, H, W = x.shape
    y = torch.empty((B, cout, H, W), device=x.device, dtype=torch.float32) if out is None else out
    if res is not None and not res.is_contiguous():
        res = res.contiguous()
    if max_workgroups is not None and not isinstance(upk, WinoF16x2):
        raise RuntimeError("max_workgroups is K10h's grid: the operand of this launch is K10's float32 image")
    if cout_blocks is not None and not isinstance(upk, WinoF16x2):
        raise RuntimeError("cout_blocks is K10h's work item: the operand of this launch is K10's float32 image")
    if isinstance(upk, WinoF16x2) and upk.f32 is not None and not wino_f16x2_wins(B, cin, cout, H, W, x.device):
        upk = upk.f32
    split = isinstance(upk, WinoF16x2)
    a = WinoArgs()
    a.x, a.y = _f32(x, "x"), _f32(y, "y")
    a.upk = _ptr(upk.image, "upk") if split else _f32(upk, "upk")
    a.shift = _f32(shift, "shift") if shift is not None else None
    a.res = _f32(res, "res") if res is not None else None
    a.batch, a.cin, a.cout, a.H, a.W = B, cin, cout, H, W
    a.act, a.res_first, a.tile_hint, a.slope = ACT2D[act], 1 if res_first else 0, int(tile_hint), float(slope)
    if (upk.cout, upk.cin) != (cout, cin) if split else upk.numel() != load().occd_wino_packed_floats(cout, cin):
        raise RuntimeError("packed Winograd weights do not match (cout, cin)")
    if _PROFILING:
        set_tag("%d>%d @%dx%dx%d" % (cin, cout, B, H, W))
    if split:
        if max_workgroups is None:
            max_workgroups = 0 if WINO_PERSIST and cout_blocks != 2 else -1
        if cout_blocks is None:
            pair = wino_cout_pair_wins(B, cin, cout, H, W) if WINO_COUT_PAIR is None else WINO_COUT_PAIR
            cout_blocks = 2 if pair and max_workgroups == -1 else 1
        _check(load().occd_wino_conv3x3_f16x2_fwd_form(ctypes.byref(a), int(max_workgroups), int(cout_blocks), _stream()),
               "occd_wino_conv3x3_f16x2_fwd_form")
    else:
        _check(load().occd_wino_conv3x3_fwd(ctypes.byref(a), _stream()), "occd_wino_conv3x3_fwd")
    return y


def pw_pack_weights(w, scale=None):
    """(Cout, Cin[, 1, 1]) 1x1-conv weight (+ per-cout scale) -> packed A operand of K11."""
    cout, cin = w.shape[0], w.shape[1]
    n = load().occd_pw_packed_floats(cout, cin)
    if n <= 0 or w.numel() != cout * cin:
        raise RuntimeError("pw_pack_weights needs a (Cout, Cin[, 1, 1]) weight")
    wc = w.detach().float().reshape(cout, cin).contiguous()
    wpk = torch.empty(n, device=w.device, dtype=torch.float32)
    sc = scale.detach().float().contiguous() if scale is not None else None
    _check(load().occd_pw_pack_weights(_f32(wc, "w"), _f32(sc, "scale") if sc is not None else None, _f32(wpk, "wpk"),
                                       cout, cin, _stream()), "occd_pw_pack_weights")
    return wpk


def conv1x1(x, wpk, cout, shift=None, act=None, slope=0.01, gate=None, res=None, tile_hint=0, out=None, nhwc=False):
    """K11: act(conv1x1(x * gate, w * scale) + shift) (+ res) on (B, Cin, *spatial) float32, one launch.
    nhwc=True: the result is stored pixel-major (B, *spatial, ceil4(Cout)) and returned as its logical (B, Cout, *spatial)
    view (channels-last strides): what the 2D->3D lift gathers from."""
    if not x.is_contiguous():
        x = x.contiguous()
    B, cin = x.shape[0], x.shape[1]
    sp = tuple(x.shape[2:])
    N = 1
    for d in sp:
        N *= d
    ocs = round_up(cout, 4) if nhwc else 0
    if nhwc:
        y = torch.empty((B,) + sp + (ocs,), device=x.device, dtype=torch.float32)
    else:
        y = torch.empty((B, cout) + sp, device=x.device, dtype=torch.float32) if out is None else out
    if res is not None and not res.is_contiguous():
        res = res.contiguous()
    if gate is not None:
        gate = gate.reshape(B, cin)
        if not gate.is_contiguous():
            gate = gate.contiguous()
    if wpk.numel() != load().occd_pw_packed_floats(cout, cin):
        raise RuntimeError("packed 1x1 weights do not match (cout, cin)")
    a = PwArgs()
    a.x, a.wpk, a.y = _f32(x, "x"), _f32(wpk, "wpk"), _f32(y, "y")
    a.shift = _f32(shift, "shift") if shift is not None else None
    a.gate = _f32(gate, "gate") if gate is not None else None
    a.res = _f32(res, "res") if res is not None else None
    a.N, a.batch, a.cin, a.cout = N, B, cin, cout
    a.act, a.tile_hint, a.slope, a.out_nhwc_cs = ACT2D[act], int(tile_hint), float(slope), ocs
    if _PROFILING:
        set_tag("%d>%d @%dx%d" % (cin, cout, B, N))
    _check(load().occd_pw_conv_fwd(ctypes.byref(a), _stream()), "occd_pw_conv_fwd")
    if nhwc:
        nd = len(sp)
        return y[..., :cout].permute(0, nd + 1, *range(1, nd + 1))
    return y


def dwconv2d_same(x, w, scale, shift, stride, act=None):
    """Depthwise conv with TensorFlow SAME padding + per-channel affine + activation, (B, C, H, W) float32."""
    if not x.is_contiguous():
        x = x.contiguous()
    B, C, H, W = x.shape
    k = w.shape[-1]
    Ho, Wo = -(-H // stride), -(-W // stride)
    pad_h = max((Ho - 1) * stride + k - H, 0)
    pad_w = max((Wo - 1) * stride + k - W, 0)
    y = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
    wc = w if w.is_contiguous() else w.contiguous()
    if _PROFILING:
        set_tag("%d k%d s%d @%dx%dx%d" % (C, k, stride, B, H, W))
    _check(load().occd_dwconv2d_nchw(_f32(x, "x"), _f32(wc, "w"), _f32(scale, "scale") if scale is not None else None,
                                     _f32(shift, "shift") if shift is not None else None, _f32(y, "y"), B, C, H, W, k,
                                     stride, pad_h // 2, pad_w // 2, Ho, Wo, ACT2D[act], _stream()),
           "occd_dwconv2d_nchw")
    return y


def depthnet_gate(mlp, se, images, sps=None, intrins=None, factor=1000.0):
    """(images, C) gate of DepthNet's camera-aware SE layer in one launch (occd_depthnet_gate): `mlp` = Mlp(1, C, C), `se` =
    SELayer(C); the scaled pixel size comes from `sps` (images,) or is derived from `intrins` (images, 4, 4) pinhole
    matrices (float32, dense)."""
    C = mlp.fc2.out_features

    def f(t):
        t = t.detach().float()
        return t if t.is_contiguous() else t.contiguous()
    gate = torch.empty((images, C), device=mlp.fc1.weight.device, dtype=torch.float32)
    if (sps is None) == (intrins is None):
        raise RuntimeError("depthnet_gate: give exactly one of sps / intrins")
    if intrins is not None:
        intr = f(intrins).reshape(images, -1)
        if intr.shape[1] < 6:
            raise RuntimeError("depthnet_gate: intrinsics need at least 6 floats per image")
        sp, ip, stride = None, _f32(intr, "intrins"), intr.shape[1]
    else:
        sv = f(sps).reshape(-1)
        if sv.numel() != images:
            raise RuntimeError("depthnet_gate: one scaled pixel size per image")
        sp, ip, stride = _f32(sv, "sps"), None, 0
    ws = [f(mlp.fc1.weight).reshape(-1), f(mlp.fc1.bias), f(mlp.fc2.weight), f(mlp.fc2.bias),
          f(se.conv_reduce.weight).reshape(C, C), f(se.conv_reduce.bias), f(se.conv_expand.weight).reshape(C, C),
          f(se.conv_expand.bias)]
    if _PROFILING:
        set_tag("%d @%d" % (C, images))
    _check(load().occd_depthnet_gate(sp, ip, stride, float(factor), *[_f32(w, "w") for w in ws], gate.data_ptr(), images, C,
                                     _stream()), "occd_depthnet_gate")
    return gate


def stem_conv3x3(x, w, scale, shift, stride, act=None):
    """conv3x3 (TensorFlow SAME padding, stride 1 / 2) of a 3-channel image + per-channel affine + activation in one launch
    (occd_stem_conv3x3_nchw): the EfficientNet stem."""
    if x.dim() != 4 or x.shape[1] != 3 or tuple(w.shape[1:]) != (3, 3, 3):
        raise RuntimeError("stem_conv3x3: x must be (B, 3, H, W) and w (cout, 3, 3, 3)")
    x = x if x.is_contiguous() else x.contiguous()
    B, _, H, W = x.shape
    cout = w.shape[0]
    Ho, Wo = -(-H // stride), -(-W // stride)
    pad_h = max((Ho - 1) * stride + 3 - H, 0)
    pad_w = max((Wo - 1) * stride + 3 - W, 0)
    y = torch.empty((B, cout, Ho, Wo), device=x.device, dtype=torch.float32)
    wc = w.detach().float()
    wc = wc if wc.is_contiguous() else wc.contiguous()
    if _PROFILING:
        set_tag("3>%d s%d @%dx%dx%d" % (cout, int(stride), B, H, W))
    _check(load().occd_stem_conv3x3_nchw(_f32(x, "x"), _f32(wc, "w"), _f32(scale, "scale") if scale is not None else None,
                                         _f32(shift, "shift") if shift is not None else None, y.data_ptr(), B, H, W, cout,
                                         int(stride), pad_h // 2, pad_w // 2, Ho, Wo, ACT2D[act], _stream()),
           "occd_stem_conv3x3_nchw")
    return y


def _same_geometry(H, W, k, stride):
    Ho, Wo = -(-H // stride), -(-W // stride)
    pad_h = max((Ho - 1) * stride + k - H, 0)
    pad_w = max((Wo - 1) * stride + k - W, 0)
    return Ho, Wo, pad_h // 2, pad_w // 2


class _DwConvSameFn(torch.autograd.Function):
    """Depthwise convolution with TensorFlow SAME padding, forward / data gradient / weight gradient on the HIP kernels
    (csrc/nchw2d.hip); under autocast it computes in float32 (HBM-bound either way)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, stride):
        x = x.contiguous()
        y = dwconv2d_same(x, w.detach(), None, None, stride, None)
        ctx.save_for_backward(x, w)
        ctx.stride = stride
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        stride = ctx.stride
        B, C, H, W = x.shape
        k = w.shape[-1]
        Ho, Wo, pt, pl = _same_geometry(H, W, k, stride)
        gy = gy.float().contiguous()
        wc = w.detach().float().contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _check(load().occd_dwconv2d_bwd_data_nchw(_f32(gy, "gy"), _f32(wc, "w"), _f32(dx, "dx"), B, C, H, W, k, stride,
                                                      pt, pl, Ho, Wo, _stream()), "occd_dwconv2d_bwd_data_nchw")
        if ctx.needs_input_grad[1]:
            n = load().occd_dwconv2d_bwd_weight_workspace_floats(B, C, k, Ho, Wo)
            ws = torch.empty(n, device=x.device, dtype=torch.float32)
            dw = torch.empty_like(wc)
            _check(load().occd_dwconv2d_bwd_weight_nchw(_f32(x, "x"), _f32(gy, "gy"), _f32(dw, "dw"), _f32(ws, "ws"), B, C,
                                                        H, W, k, stride, pt, pl, Ho, Wo, _stream()),
                   "occd_dwconv2d_bwd_weight_nchw")
        return dx, dw, None


def dwconv2d_same_autograd(x, w, stride):
    """Differentiable depthwise SAME convolution (training path of the EfficientNet blocks)."""
    return _DwConvSameFn.apply(x, w, int(stride))


class _SwishFn(torch.autograd.Function):
    """x * sigmoid(x) with a one-pass forward (affine_act) and a one-pass backward (occd_swish_bwd): 2 launches per
    site instead of the 6 of the autograd graph of `x * torch.sigmoid(x)` (training path of the EfficientNet blocks)."""

    @staticmethod
    def forward(ctx, x):
        xc = x.detach()
        if not xc.is_contiguous():
            xc = xc.contiguous()
        ctx.save_for_backward(xc)
        B, C = (xc.shape[0], xc.shape[1]) if xc.dim() >= 2 else (1, 1)
        return affine_act(xc.reshape(1, 1, -1) if B * C > 65535 or xc.dim() < 2 else xc, None, None, "swish",
                          out=torch.empty_like(xc)).reshape(x.shape)

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        g = gy.float().contiguous()
        gx = torch.empty_like(x)
        _check(load().occd_swish_bwd(_f32(x, "x"), _f32(g, "gy"), _f32(gx, "gx"), x.numel(), _stream()), "occd_swish_bwd")
        return gx


def swish_autograd(x):
    """Differentiable swish on a float32 CUDA tensor (see _SwishFn)."""
    return _SwishFn.apply(x)


class _UpCatFn(torch.autograd.Function):
    """cat([F.interpolate(x, skip's size, bilinear, align_corners=True), skip], 1) with the one-pass HIP forward
    (upsample_cat_kernel) -- ATen needs an upsample pass (0.33 ms per call at the high-resolution levels) and a concat
    copy -- and ATen's upsample backward on the matching gradient slice."""

    @staticmethod
    def forward(ctx, x, skip):
        ctx.x_shape = tuple(x.shape)
        ctx.size = tuple(skip.shape[2:])
        return upsample_bilinear_cat(x.detach().float(), skip.detach().float())

    @staticmethod
    def backward(ctx, g):
        C = ctx.x_shape[1]
        gx = gs = None
        if ctx.needs_input_grad[0]:
            gx = torch.ops.aten.upsample_bilinear2d_backward(g[:, :C].contiguous(), list(ctx.size), list(ctx.x_shape), True,
                                                             None, None)
        if ctx.needs_input_grad[1]:
            gs = g[:, C:]
        return gx, gs


class _UpCatClFn(torch.autograd.Function):
    """Channels-last twin of _UpCatFn for the bf16-mode decoder: x, skip and the result are logical (B, C, H, W) tensors in
    channels_last memory; forward = one launch (occd_upsample_bilinear_cat_nhwc), backward of the resized part = one gather
    launch (occd_upsample_bilinear_nhwc_bwd; ATen's nhwc backward scatters with atomics), the skip gradient is a view."""

    @staticmethod
    def forward(ctx, x, skip):
        B, C, h, w = x.shape
        Cs, H, W = skip.shape[1], skip.shape[2], skip.shape[3]
        xr = x.detach().float().permute(0, 2, 3, 1).contiguous()
        sr = skip.detach().float().permute(0, 2, 3, 1).contiguous()
        out = torch.empty((B, H, W, C + Cs), device=x.device, dtype=torch.float32)
        _check(load().occd_upsample_bilinear_cat_nhwc(_f32(xr, "x"), _f32(sr, "skip"), _f32(out, "out"), B, C, Cs, h, w, H, W,
                                                      _stream()), "occd_upsample_bilinear_cat_nhwc")
        ctx.geom = (B, C, Cs, h, w, H, W)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        B, C, Cs, h, w, H, W = ctx.geom
        gr = g.float().permute(0, 2, 3, 1)
        if not gr.is_contiguous():
            gr = gr.contiguous()
        gx = gs = None
        if ctx.needs_input_grad[0]:
            gxr = torch.empty((B, h, w, C), device=g.device, dtype=torch.float32)
            _check(load().occd_upsample_bilinear_nhwc_bwd(_f32(gr, "gout"), _f32(gxr, "gx"), B, C, C + Cs, h, w, H, W,
                                                          _stream()), "occd_upsample_bilinear_nhwc_bwd")
            gx = gxr.permute(0, 3, 1, 2)
        if ctx.needs_input_grad[1]:
            gs = gr[..., C:].permute(0, 3, 1, 2)
        return gx, gs


def upsample_bilinear_cat_cl_autograd(x, skip):
    return _UpCatClFn.apply(x, skip)


def upsample_bilinear_cat_autograd(x, skip):
    return _UpCatFn.apply(x, skip)


class _Conv3x3Fn(torch.autograd.Function):
    """Differentiable nn.Conv2d(3x3, stride 1, padding 1) on K10 (SURVEY 8(f) rows N1 + N3: the 2-D decoder in the training
    step).  forward = K10; data gradient = K10 on dL/dy with the 180-degree rotated, channel-transposed kernel (a 3x3 / pad 1
    convolution is its own transpose up to that); weight / bias gradient = the backend's wgrad (MIOpen implicit GEMM).
    MIOpen's fp32 forward / data-gradient choice for these shapes is the VALU Winograd kernel: 32 ms of a config-2 step."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w, b):
        y = conv2d_3x3_fused(x, wino_pack_weights(w.detach()), w.shape[0], b.detach() if b is not None else None)
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return y

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.float().contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            wt = w.detach().flip(2, 3).transpose(0, 1).contiguous()          # (cin, cout, 3, 3), rotated
            dx = conv2d_3x3_fused(gy, wino_pack_weights(wt), w.shape[1])
        want_b = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_b:
            _, dw, db = torch.ops.aten.convolution_backward(gy, x, w.detach(), [w.shape[0]] if want_b else None, [1, 1], [1, 1],
                                                            [1, 1], False, [0, 0], 1, [False, True, want_b])
            if not ctx.needs_input_grad[1]:
                dw = None
        return dx, dw, db


def conv2d_3x3_autograd(x, w, b=None):
    """Differentiable 3x3 / stride 1 / padding 1 convolution, (B, Cin, H, W) float32 CUDA tensors."""
    return _Conv3x3Fn.apply(x, w, b)


def softmax_nchw(x):
    """softmax over dim 1 of a contiguous float32 (B, C, *spatial) GPU tensor (one HIP launch)."""
    if not x.is_contiguous():
        x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    y = torch.empty_like(x)
    if _PROFILING:
        set_tag("%d @%dx%d" % (C, B, x.numel() // (B * C)))
    _check(load().occd_softmax_nchw(_f32(x, "x"), _f32(y, "y"), B, C, x.numel() // (B * C), _stream()), "occd_softmax_nchw")
    return y


def dwconv2d_same_pool(x, w, scale, shift, stride, act=None):
    """dwconv2d_same that also returns the squeeze-excite pooling partials (B*C, nblk) and the plane size Ho*Wo.
    x: dense, or (B, C, H, W) planes on a padded pitch (the view of an expand GEMM's `padded_rows` result)."""
    B, C, H, W = x.shape
    xps = x.stride(1)
    if not (x.stride(3) == 1 and x.stride(2) == W and xps >= H * W and (B == 1 or x.stride(0) == C * xps)):
        x = x.contiguous()
        xps = H * W
    k = w.shape[-1]
    Ho, Wo = -(-H // stride), -(-W // stride)
    pad_h = max((Ho - 1) * stride + k - H, 0)
    pad_w = max((Wo - 1) * stride + k - W, 0)
    y = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
    nblk = load().occd_dwconv2d_pool_blocks(Ho, Wo)
    part = torch.empty((B * C, nblk), device=x.device, dtype=torch.float32)
    wc = w if w.is_contiguous() else w.contiguous()
    if x.dtype != torch.float32 or not x.is_cuda:
        raise RuntimeError("dwconv2d_same_pool: x must be a float32 GPU tensor")
    if _PROFILING:
        set_tag("%d k%d s%d @%dx%dx%d" % (C, k, stride, B, H, W))
    _check(load().occd_dwconv2d_pool_nchw(x.data_ptr(), _f32(wc, "w"), _f32(scale, "scale") if scale is not None else None,
                                          _f32(shift, "shift") if shift is not None else None, _f32(y, "y"),
                                          _f32(part, "pool_part"), B, C, H, W, k, stride, pad_h // 2, pad_w // 2, Ho, Wo,
                                          ACT2D[act], xps, _stream()), "occd_dwconv2d_pool_nchw")
    return y, part, Ho * Wo


def se_gate(part, plane_size, batch, w_reduce, b_reduce, w_expand, b_expand):
    """Squeeze-excite gate (B, C) from the pooling partials of dwconv2d_same_pool (two small launches)."""
    C = part.shape[0] // batch
    Cr = w_reduce.shape[0]
    wr = w_reduce.detach().reshape(Cr, C).contiguous()
    we = w_expand.detach().reshape(C, Cr).contiguous()
    r = torch.empty((batch, Cr), device=part.device, dtype=torch.float32)
    gate = torch.empty((batch, C), device=part.device, dtype=torch.float32)
    if _PROFILING:
        set_tag("%d>%d>%d @%dx%d" % (C, Cr, C, batch, int(plane_size)))
    _check(load().occd_se_gate(_f32(part, "pool_part"), _f32(wr, "w_reduce"), _f32(b_reduce.detach().contiguous(), "b_reduce"),
                               _f32(we, "w_expand"), _f32(b_expand.detach().contiguous(), "b_expand"), _f32(r, "r"),
                               _f32(gate, "gate"), batch, C, Cr, part.shape[1], int(plane_size), _stream()), "occd_se_gate")
    return gate


def plane_reduce(a, b=None):
    """(planes,) sums over the trailing plane of `a` ((..., H, W) dense), or of a * b when b is given (occd_plane_reduce)."""
    a = a if a.is_contiguous() else a.contiguous()
    S = a.shape[-2] * a.shape[-1]
    planes = a.numel() // S
    if b is not None:
        b = b if b.is_contiguous() else b.contiguous()
        if b.shape != a.shape:
            raise RuntimeError("plane_reduce: operands must have the same shape")
    out = torch.empty(planes, device=a.device, dtype=torch.float32)
    _check(load().occd_plane_reduce(_f32(a, "a"), _f32(b, "b") if b is not None else None, out.data_ptr(), planes, S, _stream()),
           "occd_plane_reduce")
    return out


class _SqueezeExciteFn(torch.autograd.Function):
    """Training: geffnet's SqueezeExcite -- out = x * sigmoid(We swish(Wr mean_hw(x) + br) + be) -- forward and backward on the
    HIP passes of csrc/se2d.hip (4 + 4 launches instead of the ~22 of the autograd graph; deterministic)."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, w_reduce, b_reduce, w_expand, b_expand):
        x = x if x.is_contiguous() else x.contiguous()
        B, C, H, W = x.shape
        Cr = w_reduce.shape[0]
        sums = plane_reduce(x)
        wr = w_reduce.detach().reshape(Cr, C).contiguous()
        we = w_expand.detach().reshape(C, Cr).contiguous()
        br, be = b_reduce.detach().contiguous(), b_expand.detach().contiguous()
        r = torch.empty((B, Cr), device=x.device, dtype=torch.float32)
        gate = torch.empty((B, C), device=x.device, dtype=torch.float32)
        _check(load().occd_se_gate(sums.data_ptr(), _f32(wr, "w_reduce"), _f32(br, "b_reduce"), _f32(we, "w_expand"),
                                   _f32(be, "b_expand"), r.data_ptr(), gate.data_ptr(), B, C, Cr, 1, H * W, _stream()),
               "occd_se_gate")
        out = affine_act(x.view(1, B * C, H, W), gate.view(-1), None, out=torch.empty_like(x).view(1, B * C, H, W))
        ctx.save_for_backward(x, sums, gate, r, wr, br, we)
        return out.view(B, C, H, W)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gout):
        x, sums, gate, r, wr, br, we = ctx.saved_tensors
        B, C, H, W = x.shape
        Cr = wr.shape[0]
        gout = gout.float()
        gout = gout if gout.is_contiguous() else gout.contiguous()
        gg = plane_reduce(gout, x)
        dev = x.device
        dz = torch.empty((B, Cr), device=dev, dtype=torch.float32)
        gm = torch.empty((B, C), device=dev, dtype=torch.float32)
        gwr = torch.empty((Cr, C), device=dev, dtype=torch.float32)
        gbr = torch.empty(Cr, device=dev, dtype=torch.float32)
        gwe = torch.empty((C, Cr), device=dev, dtype=torch.float32)
        gbe = torch.empty(C, device=dev, dtype=torch.float32)
        _check(load().occd_se_bwd(gg.data_ptr(), gate.data_ptr(), sums.data_ptr(), r.data_ptr(), wr.data_ptr(), br.data_ptr(),
                                  we.data_ptr(), dz.data_ptr(), gm.data_ptr(), gwr.data_ptr(), gbr.data_ptr(), gwe.data_ptr(),
                                  gbe.data_ptr(), B, C, Cr, H * W, _stream()), "occd_se_bwd")
        gm.mul_(1.0 / (H * W))                                     # d loss / d x through the mean: + gm / S on every pixel
        gx = affine_act(gout.view(1, B * C, H, W), gate.view(-1), gm.view(-1), out=torch.empty_like(x).view(1, B * C, H, W))
        return gx.view(B, C, H, W), gwr.view(Cr, C, 1, 1), gbr, gwe.view(C, Cr, 1, 1), gbe


SE_TRAIN_MAX_IMAGES = 16
# OCCDEPTH_TRAIN_SE=0 restores the autograd graph of the SE blocks in training (A/B)
SE_TRAIN = os.environ.get("OCCDEPTH_TRAIN_SE", "1") == "1"


def squeeze_excite_autograd_ok(se, x):
    return (SE_TRAIN and x.is_cuda and x.dim() == 4 and x.shape[0] <= SE_TRAIN_MAX_IMAGES
            and (x.dtype == torch.float32 or (torch.is_autocast_enabled() and x.dtype in (torch.bfloat16, torch.float16)))
            and se.conv_reduce.bias is not None and se.conv_expand.bias is not None
            and 2 * x.shape[0] * se.conv_reduce.out_channels * 4 + x.shape[0] * 1024 <= 64 * 1024)


def squeeze_excite_autograd(se, x):
    return _SqueezeExciteFn.apply(x, se.conv_reduce.weight, se.conv_reduce.bias, se.conv_expand.weight, se.conv_expand.bias)


def upsample_bilinear_cat(x, skip):
    """cat([bilinear(x, skip's size, align_corners=True), skip], dim=1) in one pass."""
    if not x.is_contiguous():
        x = x.contiguous()
    if not skip.is_contiguous():
        skip = skip.contiguous()
    B, C, h, w = x.shape
    Cs, H, W = skip.shape[1], skip.shape[2], skip.shape[3]
    out = torch.empty((B, C + Cs, H, W), device=x.device, dtype=torch.float32)
    _check(load().occd_upsample_bilinear_cat_nchw(_f32(x, "x"), _f32(skip, "skip"), _f32(out, "out"), B, C, Cs, h, w,
                                                  H, W, _stream()), "occd_upsample_bilinear_cat_nchw")
    return out


def upconv_gather(z, cout, size, batch_inner=False, skip=None, wskip=None, shift=None, slope=0.01):
    """sum over the 9 taps of shift_t(bilinear_up(z_t)): z (B, 9 * cout, h, w) -> (B, cout, H, W), size = (H, W).
    With z = conv1x1(x, W9) this is conv3x3(pad 1)(bilinear_up(x, align_corners=True)) (see occd_upconv_gather_nchw).
    batch_inner: z is (9 * cout, B, h, w) -- the result of ONE GEMM over the pixels of all images."""
    # dense, or planes (the rows of the tap GEMM's result) on a padded pitch (`padded_rows`): the strides travel
    if not (z.stride(3) == 1 and z.stride(2) == z.shape[3] and z.stride(0) > 0 and z.stride(1) > 0 and z.dtype == torch.float32):
        z = z.contiguous()
    if batch_inner:
        c9, B, h, w = z.shape
        zcs, zbs = z.stride(0), z.stride(1)
        ok = zbs == h * w and zcs >= B * h * w
    else:
        B, c9, h, w = z.shape
        zcs, zbs = z.stride(1), z.stride(0)
        ok = zcs >= h * w and zbs >= c9 * zcs
    if not ok or not z.is_cuda:
        raise RuntimeError("upconv_gather: z must be a GPU tensor, dense or with planes on a padded pitch")
    zp = z.data_ptr()
    if c9 != 9 * cout:
        raise RuntimeError("upconv_gather: z must have 9 * cout channels")
    H, W = int(size[0]), int(size[1])
    out = torch.empty((B, cout, H, W), device=z.device, dtype=torch.float32)
    if _PROFILING:
        set_tag("%d taps9 @%dx%dx%d>%dx%d" % (cout, B, h, w, H, W))
    if skip is not None:
        # fused tail of the level: + conv3x3 over the (<= 4) skip channels + shift, LeakyReLU (occd_upconv_gather_skip_nchw)
        sk = skip if skip.is_contiguous() else skip.contiguous()
        _check(load().occd_upconv_gather_skip_nchw(zp, _f32(sk, "skip"), _f32(wskip, "wskip"), _f32(shift, "shift"),
                                                   _f32(out, "out"), B, cout, sk.shape[1], h, w, H, W, zcs, zbs, float(slope),
                                                   _stream()), "occd_upconv_gather_skip_nchw")
        return out
    _check(load().occd_upconv_gather_nchw(zp, _f32(out, "out"), B, cout, h, w, H, W, zcs, zbs, _stream()),
           "occd_upconv_gather_nchw")
    return out


def project_voxels(cam_E, cam_k, vox_origin, voxel_size, grid_dims, img_w, img_h, device="cuda", with_z=False):
    """GPU `vox2pix` (pattern 0): -> projected_pix (N, 1, 2) int64, fov_mask (N, 1) bool [, pix_z (N,) float32]."""
    import numpy as np
    e = np.ascontiguousarray(np.asarray(cam_E, dtype=np.float64).reshape(16))
    k = np.ascontiguousarray(np.asarray(cam_k, dtype=np.float64).reshape(9))
    o = np.ascontiguousarray(np.asarray(vox_origin, dtype=np.float64).reshape(3))
    X, Y, Z = (int(v) for v in grid_dims)
    n = X * Y * Z
    pix = torch.empty((n, 1, 2), dtype=torch.int64, device=device)
    fov = torch.empty((n, 1), dtype=torch.bool, device=device)
    z = torch.empty((n,), dtype=torch.float32, device=device) if with_z else None
    _check(load().occd_project_voxels(e.ctypes.data, k.ctypes.data, o.ctypes.data, float(voxel_size), X, Y, Z,
                                      int(img_w), int(img_h), _ptr(pix, "pix"), _ptr(fov.view(torch.uint8), "fov"),
                                      _ptr(z, "pix_z") if z is not None else None, _stream()), "occd_project_voxels")
    return (pix, fov, z) if with_z else (pix, fov)


def vox2pix(cam_E, cam_k, ida, vox_origin, voxel_size, dims, img_wh, with_z=False):
    """The reference dataset's voxel -> pixel tables for a whole batch, on the GPU (occd_vox2pix, pattern 0): cam_E
    (B, V, 4, 4) / cam_k (B, V, 3, 3) float64 and ida (B, V, 4, 4) float32 (or None: no flip) device tensors, the grid
    dims = (X, Y, Z) of `voxel_size` metres from `vox_origin`, an image of img_wh = (W, H).  Returns projected_pix
    (B, V, N, 1, 2) int64 and fov_mask (B, V, N, 1) bool [, pix_z (B, V, N) float32]: per (b, v) exactly
    `project_voxels`, then x' = W - 1 - x for every voxel of a view with ida[b, v, 0, 0] < 0 (kitti_dataset.py:388).
    Capture-safe: the flip flag is read on the device."""
    if cam_E.dim() != 4:
        raise RuntimeError("cam_E must be (batch, views, 4, 4)")
    B, V = (int(d) for d in cam_E.shape[:2])
    _check_calibration(B, V, cam_E, cam_k, ida)
    X, Y, Z = (int(d) for d in dims)
    n = X * Y * Z
    dev = cam_E.device
    pix = torch.empty((B, V, n, 1, 2), dtype=torch.int64, device=dev)
    fov = torch.empty((B, V, n, 1), dtype=torch.bool, device=dev)
    z = torch.empty((B, V, n), dtype=torch.float32, device=dev) if with_z else None
    a = Vox2PixArgs()
    a.cam_E, a.cam_k = cam_E.data_ptr(), cam_k.data_ptr()
    a.ida = ida.data_ptr() if ida is not None else None
    a.pix, a.fov = pix.data_ptr(), fov.data_ptr()
    a.pix_z = z.data_ptr() if z is not None else None
    for j, o in enumerate(vox_origin):
        a.vox_origin[j] = float(o)
    a.voxel_size = float(voxel_size)
    a.batch, a.n_views, a.X, a.Y, a.Z = B, V, X, Y, Z
    a.img_w, a.img_h = int(img_wh[0]), int(img_wh[1])
    _check(load().occd_vox2pix(ctypes.byref(a), _stream()), "occd_vox2pix")
    return (pix, fov, z) if with_z else (pix, fov)


def argmax_labels_u16(logits, lut=None):
    """(B, C, X, Y, Z) float32 GPU logits -> the (B, X, Y, Z) volume occd_argmax_channels writes: uint16 values in an int16
    tensor (arg-max over C, first maximum wins, optionally mapped through `lut`), which `render_voxels` reads in place.
    Channels-last views returned by the eval path (rows of a possibly wider buffer) are consumed in place.  Without a
    `lut`: one launch, one allocation, capture-safe."""
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 5:
        raise RuntimeError("argmax_labels needs float32 GPU logits of shape (B, C, X, Y, Z)")
    cl = logits.permute(0, 2, 3, 4, 1)
    B, X, Y, Z, C = cl.shape
    cs = cl.stride(3)
    rows_ok = cl.stride(4) == 1 and cs >= C and cl.stride(2) == cs * Z and cl.stride(1) == cs * Z * Y and \
        cl.stride(0) == cs * Z * Y * X
    if not rows_ok:
        cl = cl.contiguous()
        cs = C
    rows = B * X * Y * Z
    out = torch.empty((B, X, Y, Z), dtype=torch.int16, device=logits.device)
    lut_t = None
    if lut is not None:
        lut_t = torch.as_tensor(lut, dtype=torch.int32).to(torch.int16).to(logits.device).contiguous()
    _check(load().occd_argmax_channels(cl.data_ptr(), rows, cs, 0, C, lut_t.data_ptr() if lut_t is not None else None,
                                       out.data_ptr(), _stream()), "occd_argmax_channels")
    return out


def argmax_labels(logits, lut=None):
    """(B, C, X, Y, Z) float32 GPU logits -> (B, X, Y, Z) int32 class volume (argmax over C, first maximum wins),
    optionally mapped through `lut` (e.g. SemanticKITTI learning_map_inv).  Channels-last views returned by the
    eval path (rows of a possibly wider buffer) are consumed in place."""
    return argmax_labels_u16(logits, lut).to(torch.int32) & 0xFFFF


_LABEL_BYTES = {torch.uint8: 1, torch.int16: 2, getattr(torch, "uint16", torch.int16): 2}


def render_voxels(labels, views, size, palette, target=None, fov=None, background=None, alpha=256,
                  bg_colour=(255, 255, 255), view_sizes=None, aux=False):
    """Ray-cast label volumes to images in one launch (occd_render_voxels; the contract is in include/occdepth_amd.h).
    labels (B, X, Y, Z) uint8 / int16 / uint16; views (B, V, 18) float32 ray generators; size = (H, W) of the canvas and
    view_sizes an optional list of V (h, w) rectangles inside it; palette (P, 3) uint8; target like labels (error mode);
    fov (B, X, Y, Z) bool / uint8; background (B, V, H, W, 3) uint8 blended with `alpha` (0..256).  All on the GPU and
    contiguous.  -> rgb (B, V, H, W, 3) uint8, and with aux also hit int32, face uint8, depth float32 (B, V, H, W)."""
    if labels.dim() != 4 or labels.dtype not in _LABEL_BYTES:
        raise RuntimeError("labels must be a (B, X, Y, Z) uint8 / int16 / uint16 volume, got %s %s"
                           % (tuple(labels.shape), labels.dtype))
    B, X, Y, Z = (int(d) for d in labels.shape)
    if views.dtype != torch.float32 or views.dim() != 3 or views.shape[0] != B or views.shape[2] != 18:
        raise RuntimeError("views must be float32 (B, V, 18), got %s %s" % (tuple(views.shape), views.dtype))
    V = int(views.shape[1])
    H, W = int(size[0]), int(size[1])
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3:
        raise RuntimeError("palette must be uint8 (P, 3)")
    dev = labels.device
    a = RenderArgs()
    a.labels, a.views, a.palette = _ptr(labels, "labels"), _ptr(views, "views"), _ptr(palette, "palette")
    a.label_bytes = _LABEL_BYTES[labels.dtype]
    if target is not None:
        if target.dtype not in _LABEL_BYTES or target.shape != labels.shape:
            raise RuntimeError("target must be a uint8 / int16 / uint16 volume with the shape of labels")
        a.target, a.target_bytes = _ptr(target, "target"), _LABEL_BYTES[target.dtype]
    if fov is not None:
        a.fov = _ptr(_byte_mask(fov, B, X * Y * Z, "fov"), "fov")
    if background is not None:
        if background.dtype != torch.uint8 or tuple(background.shape) != (B, V, H, W, 3):
            raise RuntimeError("background must be uint8 (B, V, H, W, 3) = %s" % ((B, V, H, W, 3),))
        a.background = _ptr(background, "background")
    for t, name in ((views, "views"), (palette, "palette"), (target, "target"), (fov, "fov"), (background, "background")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, labels on {dev}")
    if view_sizes is not None:
        if len(view_sizes) != V:
            raise RuntimeError("view_sizes needs one (h, w) per view")
        for i, (h, w) in enumerate(view_sizes):
            a.view_h[i], a.view_w[i] = int(h), int(w)
    rgb = torch.empty((B, V, H, W, 3), dtype=torch.uint8, device=dev)
    a.rgb = rgb.data_ptr()
    hit = face = depth = None
    if aux:
        hit = torch.empty((B, V, H, W), dtype=torch.int32, device=dev)
        face = torch.empty((B, V, H, W), dtype=torch.uint8, device=dev)
        depth = torch.empty((B, V, H, W), dtype=torch.float32, device=dev)
        a.hit, a.face, a.depth = hit.data_ptr(), face.data_ptr(), depth.data_ptr()
    a.batch, a.n_views, a.H, a.W = B, V, H, W
    a.X, a.Y, a.Z = X, Y, Z
    a.n_palette, a.alpha = int(palette.shape[0]), int(alpha)
    for i in range(3):
        a.bg_colour[i] = int(bg_colour[i])
    _check(load().occd_render_voxels(ctypes.byref(a), _stream()), "occd_render_voxels")
    return (rgb, hit, face, depth) if aux else rgb


def frame_visibility(labels, view, size, return_hit=False):
    """occd_frame_visibility (K34): which voxels of ONE frame the pixel rays of ONE view reach.  labels (X, Y, Z) uint8 /
    int16 / uint16; view (18,) float32 ray generator in grid-voxel units (render.camera_view); size = (H, W) pixels.  All
    on the GPU and contiguous.  -> visible (X, Y, Z) uint8: 1 for every voxel a ray visits up to and including its first
    occupied one (0 < label < 255), else 0; with return_hit also hit (H, W) int32, the first occupied voxel or -1 (what
    render_voxels reports).  Zeroed by the entry point itself: capture-safe.  The contract is in include/occdepth_amd.h."""
    if labels.dim() != 3 or labels.dtype not in _LABEL_BYTES:
        raise RuntimeError("labels must be one (X, Y, Z) uint8 / int16 / uint16 volume, got %s %s" % (tuple(labels.shape), labels.dtype))
    if view.dtype != torch.float32 or view.numel() != 18:
        raise RuntimeError("view must be one float32 (18,) ray generator, got %s %s" % (tuple(view.shape), view.dtype))
    if view.device != labels.device:
        raise RuntimeError(f"view is on {view.device}, labels on {labels.device}")
    H, W = int(size[0]), int(size[1])
    a = VisibilityArgs()
    a.labels, a.view, a.label_bytes = _ptr(labels, "labels"), _ptr(view, "view"), _LABEL_BYTES[labels.dtype]
    visible = torch.empty(tuple(labels.shape), dtype=torch.uint8, device=labels.device)
    a.visible = visible.data_ptr()
    hit = None
    if return_hit:
        hit = torch.empty((max(H, 0), max(W, 0)), dtype=torch.int32, device=labels.device)
        a.hit = hit.data_ptr()
    a.H, a.W = H, W
    a.X, a.Y, a.Z = (int(d) for d in labels.shape)
    _check(load().occd_frame_visibility(ctypes.byref(a), _stream()), "occd_frame_visibility")
    return (visible, hit) if return_hit else visible


def ray_metric_size(n_classes, n_thresholds):
    """The number of int64 counters occd_ray_metric adds to: rays, valid, unknown, pred_miss, gt[C], pred[C], tp[T][C],
    tp_geo[T] (the layout is in include/occdepth_amd.h)."""
    C, T = int(n_classes), int(n_thresholds)
    return RAY_COUNTERS + 2 * C + T * C + T


def ray_metric(pred, target, origins, dirs, counts, thresholds, n_classes, unknown_mode=RAY_UNKNOWN_DROP):
    """occd_ray_metric (K35): cast rays origins[b, k] + t dirs[r] through pred[b] and target[b] in one walk and add the
    outcome of every ray to `counts`.  pred, target (B, X, Y, Z) uint8 / int16 / uint16 (the widths may differ); origins
    (B, K, 3) and dirs (N, 3) float32, grid-voxel units; counts (ray_metric_size(n_classes, len(thresholds)),) int64,
    added to and never zeroed; thresholds: 1..4 floats in grid-voxel units, by value; unknown_mode RAY_UNKNOWN_DROP /
    RAY_UNKNOWN_PASS.  All tensors on the GPU and contiguous; no allocation, no host sync.  -> counts.  The contract is
    in include/occdepth_amd.h."""
    for t, name in ((pred, "pred"), (target, "target")):
        if t.dim() != 4 or t.dtype not in _LABEL_BYTES:
            raise RuntimeError("%s must be a (B, X, Y, Z) uint8 / int16 / uint16 volume, got %s %s" % (name, tuple(t.shape), t.dtype))
    if target.shape != pred.shape:
        raise RuntimeError("target %s must have the shape of pred %s" % (tuple(target.shape), tuple(pred.shape)))
    B, X, Y, Z = (int(d) for d in pred.shape)
    if origins.dtype != torch.float32 or origins.dim() != 3 or origins.shape[0] != B or origins.shape[2] != 3:
        raise RuntimeError("origins must be float32 (B, K, 3) with B = %d, got %s %s" % (B, tuple(origins.shape), origins.dtype))
    if dirs.dtype != torch.float32 or dirs.dim() != 2 or dirs.shape[1] != 3:
        raise RuntimeError("dirs must be float32 (N, 3), got %s %s" % (tuple(dirs.shape), dirs.dtype))
    thresholds = [float(t) for t in thresholds]
    if not 1 <= len(thresholds) <= RAY_MAX_THRESHOLDS:
        raise RuntimeError("1..%d thresholds, got %d" % (RAY_MAX_THRESHOLDS, len(thresholds)))
    if not 1 <= int(n_classes) <= RAY_MAX_CLASSES:
        raise RuntimeError("n_classes must be 1..%d, got %r" % (RAY_MAX_CLASSES, n_classes))
    size = ray_metric_size(n_classes, len(thresholds))
    if counts.dtype != torch.int64 or counts.numel() != size:
        raise RuntimeError("counts must hold %d int64 counters, got %s %s" % (size, tuple(counts.shape), counts.dtype))
    for t, name in ((target, "target"), (origins, "origins"), (dirs, "dirs"), (counts, "counts")):
        if t.device != pred.device:
            raise RuntimeError(f"{name} is on {t.device}, pred on {pred.device}")
    a = RayMetricArgs()
    a.pred, a.target = _ptr(pred, "pred"), _ptr(target, "target")
    a.origins, a.dirs, a.counts = _ptr(origins, "origins"), _ptr(dirs, "dirs"), _ptr(counts, "counts")
    a.batch, a.n_origins, a.n_rays = B, int(origins.shape[1]), int(dirs.shape[0])
    a.X, a.Y, a.Z = X, Y, Z
    a.pred_bytes, a.target_bytes = _LABEL_BYTES[pred.dtype], _LABEL_BYTES[target.dtype]
    a.n_classes, a.n_thresholds, a.unknown_mode = int(n_classes), len(thresholds), int(unknown_mode)
    for i, t in enumerate(thresholds):
        a.thresholds[i] = t
    _check(load().occd_ray_metric(ctypes.byref(a), _stream()), "occd_ray_metric")
    return counts


# ---- distance transform and distance-tolerant scores (K37, csrc/edt.hip) --------------------------------------------
def dist_metric_size(n_classes, max_d2):
    """The number of int64 counters occd_dist_metric adds to: counts[2][C][T + 2] (side, slot, squared distance; the
    layout is in include/occdepth_amd.h)."""
    return 2 * int(n_classes) * (int(max_d2) + 2)


def edt_scratch_bytes(batch, n_slots, dims):
    """Bytes of scratch edt_sq needs: one uint16 plane per frame and slot beside the output."""
    X, Y, Z = (int(d) for d in dims)
    return 2 * int(batch) * int(n_slots) * X * Y * Z


def dist_metric_scratch_bytes(dims):
    """Bytes of scratch dist_metric needs: two sets of EDT_CHUNK uint16 planes of ONE frame, whatever B and C
    (4 * 8 * X Y Z: 64 MiB at 256 x 256 x 32)."""
    X, Y, Z = (int(d) for d in dims)
    return 4 * EDT_CHUNK * X * Y * Z


def _edt_common(a, labels, n_classes, max_d2, scratch, need, name):
    if labels.dim() != 4 or labels.dtype not in _LABEL_BYTES:
        raise RuntimeError("%s must be a (B, X, Y, Z) uint8 / int16 / uint16 volume, got %s %s" % (name, tuple(labels.shape), labels.dtype))
    if not 1 <= int(n_classes) <= EDT_MAX_CLASSES:
        raise RuntimeError("n_classes must be 1..%d, got %r" % (EDT_MAX_CLASSES, n_classes))
    if not 1 <= int(max_d2) <= EDT_MAX_D2:
        raise RuntimeError("max_d2 must be 1..%d, got %r" % (EDT_MAX_D2, max_d2))
    if scratch.device != labels.device:
        raise RuntimeError(f"scratch is on {scratch.device}, {name} on {labels.device}")
    nbytes = scratch.numel() * scratch.element_size()
    if nbytes < need:
        raise RuntimeError("scratch must hold %d bytes, got %d" % (need, nbytes))
    a.labels, a.label_bytes = _ptr(labels, name), _LABEL_BYTES[labels.dtype]
    a.scratch, a.scratch_bytes = _ptr(scratch, "scratch"), nbytes
    a.batch, a.X, a.Y, a.Z = (int(d) for d in labels.shape)
    a.n_classes, a.max_d2 = int(n_classes), int(max_d2)


def edt_sq(labels, slots, n_classes, max_d2, out=None, scratch=None):
    """occd_edt_sq (K37): the exact truncated squared Euclidean distance transform.  labels (B, X, Y, Z) uint8 / int16 /
    uint16 on the GPU; slots: 1..32 ints in 0 .. n_classes - 1 (slot 0: the voxels with 1 <= label < n_classes, slot c:
    label == c) -> (B, len(slots), X, Y, Z) uint16 values in an int16 tensor (`.view(torch.uint16)` where torch has it):
    min(squared distance in voxels to the nearest seed of the slot, max_d2 + 1).  out / scratch: reusable buffers (scratch
    of edt_scratch_bytes(B, len(slots), dims) bytes; allocated when absent).  No host sync.  The contract is in
    include/occdepth_amd.h."""
    slots = [int(s) for s in slots]
    if not 1 <= len(slots) <= EDT_MAX_CLASSES:
        raise RuntimeError("1..%d slots, got %d" % (EDT_MAX_CLASSES, len(slots)))
    if any(not 0 <= s < int(n_classes) for s in slots):
        raise RuntimeError("slots must lie in 0..%d, got %r" % (int(n_classes) - 1, slots))
    if labels.dim() != 4:
        raise RuntimeError("labels must be a (B, X, Y, Z) uint8 / int16 / uint16 volume, got %s %s" % (tuple(labels.shape), labels.dtype))
    B, X, Y, Z = (int(d) for d in labels.shape)
    need = edt_scratch_bytes(B, len(slots), (X, Y, Z))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=labels.device)
    if out is None:
        out = torch.empty((B, len(slots), X, Y, Z), dtype=torch.int16, device=labels.device)
    if out.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or tuple(out.shape) != (B, len(slots), X, Y, Z) \
            or out.device != labels.device:
        raise RuntimeError("out must be a 16-bit (B, S, X, Y, Z) = %s tensor beside labels, got %s %s"
                           % ((B, len(slots), X, Y, Z), tuple(out.shape), out.dtype))
    a = EdtArgs()
    _edt_common(a, labels, n_classes, max_d2, scratch, need, "labels")
    a.dist, a.n_slots = _ptr(out, "out"), len(slots)
    for i, s in enumerate(slots):
        a.slots[i] = s
    _check(load().occd_edt_sq(ctypes.byref(a), _stream()), "occd_edt_sq")
    return out


def dist_metric(pred, target, counts, n_classes, max_d2, scratch, mask=None):
    """occd_dist_metric (K37): add the distance histograms of a prediction against a target to `counts`.  pred, target
    (B, X, Y, Z) uint8 / int16 / uint16 (the widths may differ); mask None or (B, X, Y, Z) uint8 / bool: with the target's
    255 it restricts the QUERIES, never the seeds; counts (dist_metric_size(n_classes, max_d2),) int64 =
    [2][C][max_d2 + 2], added to and never zeroed: side 0 counts the prediction's voxels of every slot by their squared
    distance to the target's seeds of that slot, side 1 the target's by their distance to the prediction's; scratch: any
    tensor of at least dist_metric_scratch_bytes(dims) bytes.  All on the GPU and contiguous; no allocation, no host
    sync.  -> counts.  The contract is in include/occdepth_amd.h."""
    if pred.dim() != 4 or pred.dtype not in _LABEL_BYTES:
        raise RuntimeError("pred must be a (B, X, Y, Z) uint8 / int16 / uint16 volume, got %s %s" % (tuple(pred.shape), pred.dtype))
    if target.dim() != 4 or target.dtype not in _LABEL_BYTES or target.shape != pred.shape:
        raise RuntimeError("target must be a uint8 / int16 / uint16 volume with the shape of pred %s, got %s %s"
                           % (tuple(pred.shape), tuple(target.shape), target.dtype))
    a = EdtArgs()
    size = dist_metric_size(n_classes, max_d2)
    if counts.dtype != torch.int64 or counts.numel() != size:
        raise RuntimeError("counts must hold %d int64 counters, got %s %s" % (size, tuple(counts.shape), counts.dtype))
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if mask.dtype != torch.uint8 or mask.shape != pred.shape:
            raise RuntimeError("mask must be uint8 / bool with the shape of pred %s, got %s %s" % (tuple(pred.shape), tuple(mask.shape), mask.dtype))
    _edt_common(a, pred, n_classes, max_d2, scratch, dist_metric_scratch_bytes(pred.shape[1:]), "pred")
    if mask is not None:
        a.mask = _ptr(mask, "mask")
    for t, name in ((target, "target"), (counts, "counts"), (mask, "mask")):
        if t is not None and t.device != pred.device:
            raise RuntimeError(f"{name} is on {t.device}, pred on {pred.device}")
    a.target, a.target_bytes, a.counts = _ptr(target, "target"), _LABEL_BYTES[target.dtype], _ptr(counts, "counts")
    _check(load().occd_dist_metric(ctypes.byref(a), _stream()), "occd_dist_metric")
    return counts


# ----------------------------------------------------------------------------- temporal fusion (csrc/fuse.hip)
def fuse_store(logits, rows):
    """occd_fuse_store: softmax of ONE frame's logits (C, X, Y, Z) float32 -- contiguous planes or a channels-last view of
    (X, Y, Z, cs) rows, read in place -- into `rows` (S, pitch) float32, S = X Y Z.  -> rows."""
    if logits.dtype != torch.float32 or logits.dim() < 2 or not logits.is_cuda:
        raise RuntimeError("fuse_store needs float32 GPU logits of shape (C, ...), got %s %s" % (tuple(logits.shape), logits.dtype))
    C = int(logits.shape[0])
    S = logits[0].numel()
    if rows.dim() != 2 or rows.shape[0] != S or rows.device != logits.device:
        raise RuntimeError("rows must be (S, pitch) = (%d, pitch) on %s, got %s on %s"
                           % (S, logits.device, tuple(rows.shape), rows.device))
    lay = _logit_layout(logits[None])
    if lay is None:
        logits = logits.contiguous()
        lay = (C * S, S, 1)
    _check(load().occd_fuse_store(logits.data_ptr(), _f32(rows, "rows"), S, C, lay[1], lay[2], int(rows.shape[1]), _stream()),
           "occd_fuse_store")
    return rows


def fuse_frames(rows, affines, weights, dims, n_classes, masks=None, return_prob=False):
    """occd_fuse_frames, one launch: K sources -- rows[k] (S, pitch) float32 probability rows, affines[k] the 12 float32
    coefficients that take a target voxel centre into source k's grid, weights[k], masks[k] a (S,) uint8 / bool tensor or
    None -- fused into the X x Y x Z target grid `dims`.  -> (labels, n_obs) uint8 (X, Y, Z) and the normalised
    probabilities (S, pitch) float32, or None without return_prob (the contract is in include/occdepth_amd.h)."""
    K = len(rows)
    if not 1 <= K <= FUSE_MAX_SOURCES or len(affines) != K or len(weights) != K:
        raise RuntimeError("fuse_frames takes 1..%d sources with one affine and one weight each" % FUSE_MAX_SOURCES)
    X, Y, Z = (int(d) for d in dims)
    S = X * Y * Z
    dev = rows[0].device
    pitch = int(rows[0].shape[1])
    masks = [None] * K if masks is None else list(masks)
    if len(masks) != K:
        raise RuntimeError("masks must be None or one entry (a tensor or None) per source")
    a = FuseArgs()
    for k in range(K):
        r = rows[k]
        if r.dim() != 2 or tuple(r.shape) != (S, pitch) or r.device != dev:
            raise RuntimeError("rows[%d] must be (%d, %d) on %s, got %s on %s" % (k, S, pitch, dev, tuple(r.shape), r.device))
        a.rows[k] = _f32(r, "rows[%d]" % k)
        if masks[k] is not None:
            a.masks[k] = _ptr(_byte_mask(masks[k][None], 1, S, "masks[%d]" % k), "masks[%d]" % k)
        a.weights[k] = float(weights[k])
        coef = [float(v) for v in affines[k]]
        if len(coef) != 12:
            raise RuntimeError("affines[%d] must hold 12 values (A row-major, then b)" % k)
        for i in range(12):
            a.affine[k][i] = coef[i]
    labels = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    n_obs = torch.empty((X, Y, Z), dtype=torch.uint8, device=dev)
    prob = torch.empty((S, pitch), dtype=torch.float32, device=dev) if return_prob else None
    a.labels, a.n_obs, a.prob = _ptr(labels), _ptr(n_obs), _ptr(prob)
    a.X, a.Y, a.Z, a.C, a.K, a.pitch = X, Y, Z, int(n_classes), K, pitch
    _check(load().occd_fuse_frames(ctypes.byref(a), _stream()), "occd_fuse_frames")
    return labels, n_obs, prob


# ----------------------------------------------------------------------------- sequence-level semantic map (csrc/semantic_map.hip)
_MAP_BRICK_VOX = MAP_BRICK ** 3


def _map_operands(a, votes, table, table_host, words, n_classes):
    """Fill the fields the two argument structs share; -> the number of table rows."""
    if votes.dtype != torch.int16 or votes.dim() != 3 or votes.shape[1] != _MAP_BRICK_VOX:
        raise RuntimeError("votes must be an int16 (capacity, %d, pitch) pool, got %s %s"
                           % (_MAP_BRICK_VOX, tuple(votes.shape), votes.dtype))
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != words or table.device != votes.device:
        raise RuntimeError("table must be int32 (n_bricks, %d) on %s, got %s %s on %s"
                           % (words, votes.device, tuple(table.shape), table.dtype, table.device))
    a.votes, a.table = _ptr(votes, "votes"), _ptr(table, "table")
    if table_host is not None:
        if table_host.is_cuda or table_host.dtype != torch.int32 or table_host.shape != table.shape or \
                not table_host.is_contiguous():
            raise RuntimeError("table_host must be the table's contiguous int32 copy in host memory")
        a.table_host = table_host.data_ptr()
    a.n_bricks, a.capacity = int(table.shape[0]), int(votes.shape[0])
    a.C, a.pitch = int(n_classes), int(votes.shape[2])
    return a.n_bricks


def map_integrate(votes, table, labels, dims, n_classes, mask=None, table_host=None):
    """occd_map_integrate, one launch: the frame `labels` (X Y Z entries, uint8 / int16 / uint16) votes into the bricks
    the (n, 16) int32 `table` names (slot | key | Aq | cq per row, semantic_map.brick_coefficients), inside `mask`
    (X Y Z bool / uint8 entries) when given.  votes: the int16 (capacity, 4096, pitch) pool, updated in place.  The
    contract is in include/occdepth_amd.h."""
    return _map_integrate(votes, table, labels, dims, n_classes, mask, None, table_host)


def _check_weight(t, S, name):
    """A weight volume as the kernels read it: X Y Z uint8 entries."""
    if t is not None and (not torch.is_tensor(t) or t.dtype != torch.uint8 or t.numel() != S):
        raise RuntimeError("%s must hold X Y Z = %d uint8 weights, got %s %s"
                           % (name, S, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__, getattr(t, "dtype", None)))


def _map_integrate(votes, table, labels, dims, n_classes, mask, weight, table_host):
    X, Y, Z = (int(d) for d in dims)
    if labels.dtype not in _LABEL_BYTES or labels.numel() != X * Y * Z:
        raise RuntimeError("labels must hold X Y Z = %d uint8 / int16 / uint16 entries, got %s %s"
                           % (X * Y * Z, tuple(labels.shape), labels.dtype))
    _check_weight(weight, X * Y * Z, "weight")
    a = MapFrameArgs() if weight is None else MapWeightedArgs()
    _map_operands(a, votes, table, table_host, 16, n_classes)
    a.labels, a.label_bytes = _ptr(labels, "labels"), _LABEL_BYTES[labels.dtype]
    if weight is not None:
        a.weight = _ptr(weight, "weight")
    elif mask is not None:
        a.mask = _ptr(_byte_mask(mask.reshape(1, -1), 1, X * Y * Z, "mask"), "mask")
    for t, name in ((labels, "labels"), (mask, "mask"), (weight, "weight")):
        if t is not None and t.device != votes.device:
            raise RuntimeError(f"{name} is on {t.device}, votes on {votes.device}")
    a.X, a.Y, a.Z = X, Y, Z
    if weight is None:
        _check(load().occd_map_integrate(ctypes.byref(a), _stream()), "occd_map_integrate")
    else:
        _check(load().occd_map_integrate_weighted(ctypes.byref(a), _stream()), "occd_map_integrate_weighted")
    return votes


def map_integrate_weighted(votes, table, labels, dims, n_classes, weight, table_host=None):
    """occd_map_integrate_weighted, one launch: map_integrate with a required `weight` volume (X Y Z uint8 entries) in
    place of the mask -- voxel n votes with weight[n], counters become min(v + w, 65535), weight 0 casts no vote."""
    if weight is None:
        raise RuntimeError("map_integrate_weighted needs the weight volume (map_integrate takes an optional mask)")
    return _map_integrate(votes, table, labels, dims, n_classes, None, weight, table_host)


def map_brick_labels(votes, table, n_classes, table_host=None):
    """occd_map_brick_labels: the (n, 4) int32 `table` (slot | key per row; a negative slot = not in the map) ->
    (n, 16, 16, 16) uint8 labels, 255 where a voxel has no vote or its brick is not in the map."""
    a = MapExtractArgs()
    n = _map_operands(a, votes, table, table_host, 4, n_classes)
    dense = torch.empty((n, MAP_BRICK, MAP_BRICK, MAP_BRICK), dtype=torch.uint8, device=votes.device)
    a.dense = dense.data_ptr()
    _check(load().occd_map_brick_labels(ctypes.byref(a), _stream()), "occd_map_brick_labels")
    return dense


def map_extract(votes, table, n_classes, min_obs=1, include_empty=False, table_host=None):
    """occd_map_count -> exclusive scan -> occd_map_extract: the voxels of the table's bricks with at least `min_obs`
    votes (and a label other than 0 unless include_empty), bricks in table order, voxels in (i, j, l) order ->
    coords (N, 3) int32 world voxel indices, labels (N,) uint8, n_obs (N,) int16 holding uint16 bits.  One host
    synchronisation, for N."""
    a = MapExtractArgs()
    n = _map_operands(a, votes, table, table_host, 4, n_classes)
    dev = votes.device
    a.min_obs, a.include_empty = int(min_obs), int(bool(include_empty))
    counts = torch.empty((n,), dtype=torch.int32, device=dev)
    a.counts = counts.data_ptr()
    _check(load().occd_map_count(ctypes.byref(a), _stream()), "occd_map_count")
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = (ends - counts).contiguous()
    N = int(ends[-1])
    coords = torch.empty((N, 3), dtype=torch.int32, device=dev)
    labels = torch.empty((N,), dtype=torch.uint8, device=dev)
    n_obs = torch.empty((N,), dtype=torch.int16, device=dev)
    if N:
        a.offsets, a.coords, a.labels, a.n_obs, a.n_out = offsets.data_ptr(), coords.data_ptr(), labels.data_ptr(), \
            n_obs.data_ptr(), N
        _check(load().occd_map_extract(ctypes.byref(a), _stream()), "occd_map_extract")
    return coords, labels, n_obs


def map_sample(votes, table, cells, own, dims, n_classes, Bq, dq, grid, own_mask=None, min_obs=1, exclude_self=False,
               keep_own=False, table_host=None):
    """occd_map_sample (K32), one launch: every voxel of the (X, Y, Z) = `dims` frame reads the map back.  votes: the
    int16 (capacity, 4096, pitch) pool (only read); table (n, 16) int32 (slot | key | Aq | cq per row, the frame's own
    coefficients); cells (gx, gy, gz) = `grid` int32, the table row of the brick at each cell of the frame's window or
    -1; own: the frame's own labels (X Y Z entries, uint8 / int16 / uint16) or None; own_mask: the (X Y Z) bool / uint8
    mask it voted with or None; Bq (3, 3), dq (3,) from semantic_map.sample_coefficients.  exclude_self / keep_own need
    `own`.  -> labels (X, Y, Z) uint8, n_obs (X, Y, Z) int16 holding uint16 bits.  The contract is in
    include/occdepth_amd.h."""
    return _map_sample(votes, table, cells, own, dims, n_classes, Bq, dq, grid, own_mask, None, min_obs, exclude_self, keep_own,
                       table_host)


def map_sample_weighted(votes, table, cells, own, dims, n_classes, Bq, dq, grid, own_weight=None, min_obs=1,
                        exclude_self=False, keep_own=False, table_host=None):
    """occd_map_sample_weighted, one launch: map_sample for a map of weighted votes.  own_weight: the (X Y Z) uint8
    weights the frame voted with, required by exclude_self (which retracts them) and read by nothing else.  min_obs and
    the returned n_obs are in vote units."""
    if exclude_self and own_weight is None:
        raise RuntimeError("exclude_self retracts the frame's own weights: own_weight is needed")
    return _map_sample(votes, table, cells, own, dims, n_classes, Bq, dq, grid, None, own_weight, min_obs, exclude_self, keep_own,
                       table_host, weighted=True)


def _map_sample(votes, table, cells, own, dims, n_classes, Bq, dq, grid, own_mask, own_weight, min_obs, exclude_self, keep_own,
                table_host, weighted=False):
    X, Y, Z = (int(d) for d in dims)
    S = X * Y * Z
    if cells.dtype != torch.int32 or cells.dim() != 3 or tuple(cells.shape) != tuple(int(g) for g in grid):
        raise RuntimeError("cells must be an int32 (gx, gy, gz) = %r directory, got %s %s" % (tuple(grid), tuple(cells.shape), cells.dtype))
    if own is not None and (own.dtype not in _LABEL_BYTES or own.numel() != S):
        raise RuntimeError("own must hold X Y Z = %d uint8 / int16 / uint16 entries, got %s %s" % (S, tuple(own.shape), own.dtype))
    if own is None and (exclude_self or keep_own):
        raise RuntimeError("exclude_self and keep_own need the frame's own labels")
    _check_weight(own_weight, S, "own_weight")
    Bq, dq = [int(v) for r in Bq for v in r], [int(v) for v in dq]
    if len(Bq) != 9 or len(dq) != 3 or not all(-(1 << 31) <= v < 1 << 31 for v in Bq + dq):
        raise RuntimeError("Bq must be a 3 x 3 and dq a 3-vector of int32 (semantic_map.sample_coefficients)")
    a = MapSampleWeightedArgs() if weighted else MapSampleArgs()
    _map_operands(a, votes, table, table_host, 16, n_classes)
    a.cells = _ptr(cells, "cells")
    if own is not None:
        a.own, a.label_bytes = _ptr(own, "own"), _LABEL_BYTES[own.dtype]
    else:
        a.label_bytes = 1
    if own_mask is not None:
        a.own_mask = _ptr(_byte_mask(own_mask.reshape(1, -1), 1, S, "own_mask"), "own_mask")
    if own_weight is not None:
        a.own_weight = _ptr(own_weight, "own_weight")
    for t, name in ((cells, "cells"), (own, "own"), (own_mask, "own_mask"), (own_weight, "own_weight")):
        if t is not None and t.device != votes.device:
            raise RuntimeError(f"{name} is on {t.device}, votes on {votes.device}")
    labels = torch.empty((X, Y, Z), dtype=torch.uint8, device=votes.device)
    n_obs = torch.empty((X, Y, Z), dtype=torch.int16, device=votes.device)
    a.labels, a.n_obs = labels.data_ptr(), n_obs.data_ptr()
    a.X, a.Y, a.Z = X, Y, Z
    a.gx, a.gy, a.gz = (int(g) for g in cells.shape)
    a.min_obs = int(min_obs)
    a.flags = (MAP_SAMPLE_EXCLUDE_SELF if exclude_self else 0) | (MAP_SAMPLE_KEEP_OWN if keep_own else 0)
    for i, v in enumerate(Bq):
        a.Bq[i] = v
    for i, v in enumerate(dq):
        a.dq[i] = v
    if weighted:
        _check(load().occd_map_sample_weighted(ctypes.byref(a), _stream()), "occd_map_sample_weighted")
    else:
        _check(load().occd_map_sample(ctypes.byref(a), _stream()), "occd_map_sample")
    return labels, n_obs


def map_merge(votes, src, table, table_host=None, split=0):
    """occd_map_merge (K33), one launch: votes[slot] = min(votes[slot] + src[row], 65535), counter by counter, for every
    (slot, row) of the (n, 2) int32 `table`.  votes: the int16 (capacity, 4096, pitch) pool, updated in place; src: int16
    (rows, 4096, pitch) in the same layout on the same device (another map's pool or a buffer of received rows; it must
    not overlap the destination bricks).  split: workgroups per brick, 0 = the library's choice.  n == 0 launches
    nothing.  The contract is in include/occdepth_amd.h."""
    for t, name in ((votes, "votes"), (src, "src")):
        if t.dtype != torch.int16 or t.dim() != 3 or t.shape[1] != _MAP_BRICK_VOX:
            raise RuntimeError("%s must be int16 (bricks, %d, pitch), got %s %s" % (name, _MAP_BRICK_VOX, tuple(t.shape), t.dtype))
    if src.shape[2] != votes.shape[2] or src.device != votes.device:
        raise RuntimeError("src has pitch %d on %s, votes pitch %d on %s" % (src.shape[2], src.device, votes.shape[2], votes.device))
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 2 or table.device != votes.device:
        raise RuntimeError("table must be int32 (n, 2) on %s, got %s %s on %s"
                           % (votes.device, tuple(table.shape), table.dtype, table.device))
    a = MapMergeArgs()
    a.votes, a.src = _ptr(votes, "votes"), _ptr(src, "src")
    if table_host is not None:
        if table_host.is_cuda or table_host.dtype != torch.int32 or table_host.shape != table.shape or \
                not table_host.is_contiguous():
            raise RuntimeError("table_host must be the table's contiguous int32 copy in host memory")
        a.table_host = table_host.data_ptr()
    a.n, a.capacity, a.src_capacity = int(table.shape[0]), int(votes.shape[0]), int(src.shape[0])
    a.pitch, a.split = int(votes.shape[2]), int(split)
    if a.n == 0:
        return votes
    a.table = _ptr(table, "table")
    _check(load().occd_map_merge(ctypes.byref(a), _stream()), "occd_map_merge")
    return votes


def map_render(labels, cells, views, size, palette, target=None, background=None, alpha=256, bg_colour=(255, 255, 255),
               view_sizes=None, t_max=float("inf"), skip=True, aux=False):
    """Ray-cast a brick map to images in one launch (occd_map_render, K31; the contract is in include/occdepth_amd.h).
    labels (n, 4096) (or (n, 16, 16, 16)) uint8 brick rows; cells (gx, gy, gz) int32 directory, the row of the brick at
    that cell or -1; views (V, 18) float32 ray generators in window voxel units; size = (H, W) of the canvas and
    view_sizes an optional list of V (h, w) rectangles inside it; palette (P, 3) uint8; target like labels (error mode);
    background (V, H, W, 3) uint8 blended with `alpha` (0..256); t_max: hits deeper than this are misses; skip=False
    walks absent bricks voxel by voxel (the same images, for A/B runs).  All on the GPU and contiguous.  -> rgb
    (V, H, W, 3) uint8, and with aux also hit int64 (row * 4096 + local voxel or -1), face uint8, depth float32 (V, H, W)."""
    if labels.dtype != torch.uint8 or labels.dim() not in (2, 4) or labels.shape[0] < 1 or labels[0].numel() != _MAP_BRICK_VOX:
        raise RuntimeError("labels must be uint8 (n, %d) brick rows, got %s %s" % (_MAP_BRICK_VOX, tuple(labels.shape), labels.dtype))
    if cells.dtype != torch.int32 or cells.dim() != 3:
        raise RuntimeError("cells must be an int32 (gx, gy, gz) directory, got %s %s" % (tuple(cells.shape), cells.dtype))
    if views.dtype != torch.float32 or views.dim() != 2 or views.shape[1] != 18:
        raise RuntimeError("views must be float32 (V, 18), got %s %s" % (tuple(views.shape), views.dtype))
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3:
        raise RuntimeError("palette must be uint8 (P, 3)")
    V = int(views.shape[0])
    H, W = int(size[0]), int(size[1])
    dev = labels.device
    a = MapRenderArgs()
    a.labels, a.cells, a.views, a.palette = _ptr(labels, "labels"), _ptr(cells, "cells"), _ptr(views, "views"), _ptr(palette, "palette")
    if target is not None:
        if target.dtype != torch.uint8 or target.shape != labels.shape:
            raise RuntimeError("target must be uint8 brick rows with the shape of labels")
        a.target = _ptr(target, "target")
    if background is not None:
        if background.dtype != torch.uint8 or tuple(background.shape) != (V, H, W, 3):
            raise RuntimeError("background must be uint8 (V, H, W, 3) = %s" % ((V, H, W, 3),))
        a.background = _ptr(background, "background")
    for t, name in ((cells, "cells"), (views, "views"), (palette, "palette"), (target, "target"), (background, "background")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} is on {t.device}, labels on {dev}")
    if view_sizes is not None:
        if len(view_sizes) != V:
            raise RuntimeError("view_sizes needs one (h, w) per view")
        for i, (h, w) in enumerate(view_sizes):
            a.view_h[i], a.view_w[i] = int(h), int(w)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    a.rgb = rgb.data_ptr()
    hit = face = depth = None
    if aux:
        hit = torch.empty((V, H, W), dtype=torch.int64, device=dev)
        face = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
        depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        a.hit, a.face, a.depth = hit.data_ptr(), face.data_ptr(), depth.data_ptr()
    a.gx, a.gy, a.gz = (int(d) for d in cells.shape)
    a.n_rows, a.n_views, a.H, a.W = int(labels.shape[0]), V, H, W
    a.n_palette, a.alpha = int(palette.shape[0]), int(alpha)
    a.t_max, a.flags = float(t_max), 0 if skip else 1
    for i in range(3):
        a.bg_colour[i] = int(bg_colour[i])
    _check(load().occd_map_render(ctypes.byref(a), _stream()), "occd_map_render")
    return (rgb, hit, face, depth) if aux else rgb


# ----------------------------------------------------------------------------- stereo depth targets (csrc/stereo.hip)
def _stereo_geometry(t, name, shape):
    """(B, H, W) of a GPU tensor shaped (B, 2, ..., H, W) with `shape` naming its dimensions."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (the stereo matcher has no CPU path)")
    if t.dim() != len(shape) or t.shape[1] != 2 or min(t.shape) < 1:
        raise RuntimeError(f"{name} must be a non-empty ({', '.join(shape)}) tensor, got {tuple(t.shape)}")
    return int(t.shape[0]), int(t.shape[-2]), int(t.shape[-1])


def stereo_census(gray=None, img=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """occd_stereo_census: gray (B, 2, H, W) uint8 -- or img (B, 2, 3, H, W) normalised float32, converted on the way --
    -> (gray, census); census is (B, 2, H, W) int64 holding the 64-bit words."""
    if (gray is None) == (img is None):
        raise RuntimeError("stereo_census takes either a uint8 gray pair or a normalised float32 image pair")
    a = StereoArgs()
    if img is not None:
        B, H, W = _stereo_geometry(img, "img", ("B", "2", "3", "H", "W"))
        if img.dtype != torch.float32 or img.shape[2] != 3:
            raise RuntimeError("img must be float32 (B, 2, 3, H, W), got %s %s" % (tuple(img.shape), img.dtype))
        a.img = _ptr(img, "img")
        gray = torch.empty((B, 2, H, W), dtype=torch.uint8, device=img.device)
        for c in range(3):
            a.mean[c], a.std[c] = float(mean[c]), float(std[c])
    else:
        B, H, W = _stereo_geometry(gray, "gray", ("B", "2", "H", "W"))
        if gray.dtype != torch.uint8:
            raise RuntimeError("gray must be uint8 (B, 2, H, W), got %s" % gray.dtype)
    census = torch.empty((B, 2, H, W), dtype=torch.int64, device=gray.device)
    a.gray, a.census = _ptr(gray, "gray"), census.data_ptr()
    a.batch, a.H, a.W = B, H, W
    _check(load().occd_stereo_census(ctypes.byref(a), _stream()), "occd_stereo_census")
    return gray, census


def stereo_sgm(census, max_disp=192, ida=None, p1=10, p2=120, uniqueness=95):
    """occd_stereo_sgm on census words (B, 2, H, W) int64: -> S (B, H, W, D) int16 (uint16 values <= 1020), d0 (B, H, W)
    int32, flags (B, H, W) uint8 (1 unique | 2 consistent | 4 inner), disp (B, H, W) float32 (0 = invalid).  ida
    (B, V, 4, 4) float32 or None: frame b is mirrored when ida[b, 0, 0, 0] < 0 (read on the device).  The workspace is a
    tensor of this call (nothing module-level that a captured graph could outlive)."""
    B, H, W = _stereo_geometry(census, "census", ("B", "2", "H", "W"))
    if census.dtype != torch.int64:
        raise RuntimeError("census must be int64 (B, 2, H, W), got %s" % census.dtype)
    D = int(max_disp)
    need = load().occd_stereo_workspace_bytes(B, H, W, D)
    if need < 0:
        raise ValueError("stereo_sgm: max_disp must be a multiple of 64 in 64..256 (got %d) and the images at most "
                         "65535 rows and 2^29 pixels (got %d x %d, batch %d)" % (D, H, W, B))
    if not (0 <= int(p1) <= int(p2) <= 193):
        raise ValueError("stereo_sgm: needs 0 <= p1 <= p2 <= 193 (a path value must fit a byte), got p1=%s p2=%s" % (p1, p2))
    if not (1 <= int(uniqueness) <= 100):
        raise ValueError("stereo_sgm: uniqueness must be in 1..100, got %s" % (uniqueness,))
    dev = census.device
    a = StereoArgs()
    a.census = _ptr(census, "census")
    if ida is not None:
        if ida.dtype != torch.float32 or ida.dim() != 4 or ida.shape[0] != B or tuple(ida.shape[2:]) != (4, 4):
            raise RuntimeError("ida must be float32 (B, V, 4, 4), got %s %s" % (tuple(ida.shape), ida.dtype))
        if ida.device != dev:
            raise RuntimeError(f"ida is on {ida.device}, census on {dev}")
        a.ida, a.ida_views = _ptr(ida, "ida"), int(ida.shape[1])
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    S = torch.empty((B, H, W, D), dtype=torch.int16, device=dev)
    d0 = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    flags = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    disp = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    a.workspace, a.S, a.d0, a.flags, a.disp = work.data_ptr(), S.data_ptr(), d0.data_ptr(), flags.data_ptr(), disp.data_ptr()
    a.batch, a.H, a.W, a.max_disp = B, H, W, D
    a.p1, a.p2, a.uniqueness = int(p1), int(p2), int(uniqueness)
    _check(load().occd_stereo_sgm(ctypes.byref(a), _stream()), "occd_stereo_sgm")
    return S, d0, flags, disp


def stereo_depth(disp, cam_k, cam_E):
    """occd_stereo_depth: disp (B, H, W) float32, cam_k (B, V, 3, 3) and cam_E (B, V, 4, 4) float64 device tensors, V >= 2,
    view 0 the left camera -> depth (B, H, W) float32 = fB / disp, 0 where disp is 0; fB is computed on the device."""
    if not torch.is_tensor(disp) or not disp.is_cuda or disp.dtype != torch.float32 or disp.dim() != 3:
        raise RuntimeError("disp must be a float32 (B, H, W) GPU tensor (the stereo matcher has no CPU path)")
    B, H, W = (int(d) for d in disp.shape)
    _check_calibration(B, int(cam_E.shape[1]) if cam_E.dim() == 4 else -1, cam_E, cam_k)
    if cam_E.shape[1] < 2:
        raise RuntimeError("stereo_depth needs the calibration of both cameras, got %d view(s)" % cam_E.shape[1])
    depth = torch.empty_like(disp)
    a = StereoArgs()
    a.disp, a.depth, a.cam_k, a.cam_E = _ptr(disp, "disp"), depth.data_ptr(), cam_k.data_ptr(), cam_E.data_ptr()
    a.batch, a.H, a.W, a.calib_views = B, H, W, int(cam_E.shape[1])
    _check(load().occd_stereo_depth(ctypes.byref(a), _stream()), "occd_stereo_depth")
    return depth


# ----------------------------------------------------------------------------- training-step statistics (N1 / N4)
SSC_Q32 = 4294967296.0
SSC_Q24 = 16777216.0


_ssc_scale_cache = {}


def ssc_stats_scale(C, F, device):
    """Multipliers that turn the fixed-point int64 statistics of occd_ssc_loss_stats_fwd into real sums
    (built once per (C, F, device): no host-to-device copy on the loss path after the first step)."""
    key = (int(C), int(F), str(device))
    sc = _ssc_scale_cache.get(key)
    if sc is None:
        sc = torch.ones(3 * C + 3 + F * C, dtype=torch.float64)
        sc[:2 * C] = 1.0 / SSC_Q32
        sc[3 * C + 1:3 * C + 3] = 1.0 / SSC_Q24
        sc[3 * C + 3:] = 1.0 / SSC_Q32
        sc = _ssc_scale_cache[key] = sc.to(device)
    return sc


def _logit_layout(logits):
    """(s_b, s_c, s_v) element strides of a (B, C, ...) logits tensor the loss kernels read in place: (B, C, S) planes
    (contiguous) or the 3-D stack's channels-last voxel rows (a permuted view of (B, ..., cs) rows, cs >= C); None when
    the tensor is neither (the caller makes it contiguous)."""
    B, C = logits.shape[:2]
    S = logits[0, 0].numel()
    if logits.is_contiguous():
        return C * S, S, 1
    st, sh = logits.stride(), logits.shape
    if st[1] != 1 or logits.dim() < 3:
        return None
    cs = st[-1]
    expect = cs
    for d in range(logits.dim() - 1, 1, -1):            # spatial dims must merge into one row index
        if sh[d] != 1 and st[d] != expect:
            return None
        expect *= sh[d]
    if cs < C or cs % 4 or (B > 1 and st[0] % 4) or logits.data_ptr() % 16:
        return None
    return (st[0] if B > 1 else S * cs), 1, cs


def _loss_operands(logits, target, masks, weights):
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() < 3:
        raise RuntimeError("ssc loss statistics need float32 GPU logits of shape (B, C, ...)")
    B, C = logits.shape[:2]
    S = logits[0, 0].numel()
    if target.dtype != torch.uint8 or tuple(target.shape) != (B,) + tuple(logits.shape[2:]):
        raise RuntimeError("target must be uint8 of shape (B, ...)")
    F = 0
    if masks is not None:
        if masks.dtype not in (torch.bool, torch.uint8) or masks.shape[0] != B or masks[0, 0].numel() != S:
            raise RuntimeError("frustum masks must be bool/uint8 of shape (B, F, ...)")
        F = masks.shape[1]
    if weights is not None and (weights.dtype != torch.float32 or weights.numel() != C):
        raise RuntimeError("class weights must be float32 of length C")
    return B, C, S, F


def ssc_loss_stats(logits, target, masks=None, weights=None, map_occ=False):
    """-> int64 (3C + 3 + F*C) fixed-point sums (see include/occdepth_amd.h); one pass over the logits, read in place
    whether they are (B, C, S) planes or channels-last voxel rows (`_logit_layout`)."""
    B, C, S, F = _loss_operands(logits, target, masks, weights)
    lay = _logit_layout(logits)
    if lay is None:
        logits = logits.contiguous()
        lay = (C * S, S, 1)
    stats = torch.empty(3 * C + 3 + F * C, dtype=torch.int64, device=logits.device)
    _check(load().occd_ssc_loss_stats_fwd_strided(logits.data_ptr(), _ptr(target, "target"), _ptr(masks, "masks"),
                                                  _ptr(weights, "weights"), stats.data_ptr(), B, C, S, F, int(bool(map_occ)),
                                                  lay[0], lay[1], lay[2], _stream()), "occd_ssc_loss_stats_fwd_strided")
    return stats


def ssc_loss_grad(logits, target, masks, weights, gstats, map_occ=False):
    """d loss / d logits from d loss / d sums (float32, the layout of ssc_loss_stats).  The gradient has the logits'
    layout: channels-last logits get a channels-last gradient -- a (B, C, ...) view of zero-padded (B, ..., cs) rows, which
    the convolution backward (autograd3d._to_vox) consumes without a transpose."""
    B, C, S, F = _loss_operands(logits, target, masks, weights)
    if gstats.dtype != torch.float32 or gstats.numel() != 3 * C + 3 + F * C:
        raise RuntimeError("gstats must be float32 of length 3C + 3 + F*C")
    lay = _logit_layout(logits)
    if lay is None:
        logits = logits.contiguous()
        lay = (C * S, S, 1)
    if lay[1] == 1:
        cs = round_up(C, 8)
        rows = torch.empty((B,) + tuple(logits.shape[2:]) + (cs,), dtype=torch.float32, device=logits.device)
        grad = rows[..., :C].permute(0, logits.dim() - 1, *range(1, logits.dim() - 1))
        glay, gpad = (S * cs, 1, cs), cs
    else:
        grad = torch.empty_like(logits)
        glay, gpad = lay, 0
    _check(load().occd_ssc_loss_stats_bwd_strided(logits.data_ptr(), _ptr(target, "target"), _ptr(masks, "masks"),
                                                  _ptr(weights, "weights"), _ptr(gstats, "gstats"), grad.data_ptr(), B, C, S, F,
                                                  int(bool(map_occ)), lay[0], lay[1], lay[2], glay[0], glay[1], glay[2], gpad,
                                                  _stream()), "occd_ssc_loss_stats_bwd_strided")
    return grad


def ssc_confusion(hist, target, logits=None, labels=None):
    """hist (C, C) int64 += confusion counts [target, prediction] over labelled voxels; the prediction is `labels`
    (uint8) or the arg-max of `logits` (B, C, ...; planes or channels-last rows, read in place)."""
    C = hist.shape[0]
    if hist.dtype != torch.int64 or hist.shape != (C, C) or target.dtype != torch.uint8:
        raise RuntimeError("hist must be int64 (C, C) and target uint8")
    if (logits is None) == (labels is None):
        raise RuntimeError("give exactly one of logits / labels")
    B = target.shape[0]
    S = target[0].numel()
    lay = (C * S, S, 1)
    if logits is not None:
        if logits.dtype != torch.float32 or logits.shape[:2] != (B, C) or logits[0, 0].numel() != S:
            raise RuntimeError("logits must be float32 (B, C, ...) matching target")
        lay = _logit_layout(logits)
        if lay is None:
            logits = logits.contiguous()
            lay = (C * S, S, 1)
    if labels is not None and (labels.dtype != torch.uint8 or labels.shape != target.shape):
        raise RuntimeError("labels must be uint8 with the shape of target")
    _check(load().occd_ssc_confusion_strided(logits.data_ptr() if logits is not None else None, _ptr(labels, "labels"),
                                             _ptr(target, "target"), _ptr(hist, "hist"), B, C, S, lay[0], lay[1], lay[2],
                                             _stream()), "occd_ssc_confusion_strided")
    return hist


NEED_FOV = 1                    # `need` bits of a region: the camera FOV, then mask slot i -> NEED_MASK0 << i
NEED_MASK0 = 2


def _byte_mask(t, B, S, name):
    """A (B, ...) bool / uint8 GPU mask with S entries per frame -> its contiguous uint8 view (no copy)."""
    if not torch.is_tensor(t) or t.dtype not in (torch.bool, torch.uint8) or t.shape[0] != B or t[0].numel() != S:
        raise RuntimeError(f"{name} must be a bool / uint8 tensor of shape (B, ...) matching target")
    if t.dtype == torch.bool:
        _ptr(t, name)
        t = t.view(torch.uint8)
    return t


def ssc_confusion_regions(hist, target, regions, logits=None, labels=None, masks=(), fov=None, per_frame=False):
    """hist += confusion counts [target, prediction] BY REGION, one pass (occd_ssc_confusion_regions).  target: uint8
    (B, X, Y, Z), 255 = unlabelled; the prediction is `labels` (uint8) or the arg-max of `logits` (B, C, X, Y, Z; planes
    or channels-last rows, read in place).  regions: up to 8 pairs (box, need): box = (x0, x1, y0, y1, z0, z1) voxel
    indices, half open (None: the whole grid), need = NEED_FOV | NEED_MASK0 << i ... .  masks: up to three bool / uint8
    (B, ...) tensors.  fov: a bool / uint8 (B, ...) mask, or the calibration (cam_E (B, V, 4, 4) float64, cam_k
    (B, V, 3, 3) float64, vox_origin, voxel_size, (W, H)[, views = (0,)]) from which the kernel computes the flag of
    `vox2pix(...)[1][b, v, :, 0]`, OR-ed over `views`.  hist: int64 (R, C, C), or (B, R, C, C) with per_frame."""
    R = len(regions)
    if target.dtype != torch.uint8 or target.dim() < 2:
        raise RuntimeError("target must be uint8 of shape (B, X, Y, Z)")
    B = int(target.shape[0])
    S = target[0].numel()
    dims = tuple(int(d) for d in target.shape[1:]) if target.dim() == 4 else (S, 1, 1)
    if hist.dtype != torch.int64 or hist.dim() != (4 if per_frame else 3) or hist.shape[-1] != hist.shape[-2] or \
            tuple(hist.shape[:-2]) != ((B, R) if per_frame else (R,)):
        raise RuntimeError("hist must be int64 (R, C, C), or (B, R, C, C) with per_frame")
    C = int(hist.shape[-1])
    if not 1 <= R <= MAX_REGIONS:
        raise RuntimeError(f"1..{MAX_REGIONS} regions per call, got {R}")
    if (logits is None) == (labels is None):
        raise RuntimeError("give exactly one of logits / labels")
    if len(masks) > 3:
        raise RuntimeError("at most three masks")
    a = ConfusionRegionsArgs()
    lay = (C * S, S, 1)
    if logits is not None:
        if logits.dtype != torch.float32 or logits.shape[:2] != (B, C) or logits[0, 0].numel() != S:
            raise RuntimeError("logits must be float32 (B, C, ...) matching target")
        lay = _logit_layout(logits)
        if lay is None:
            logits = logits.contiguous()
            lay = (C * S, S, 1)
        if not logits.is_cuda:
            raise RuntimeError("logits must live on the GPU (the HIP kernels have no CPU path)")
        a.logits = logits.data_ptr()
    if labels is not None:
        if labels.dtype != torch.uint8 or labels.shape != target.shape:
            raise RuntimeError("labels must be uint8 with the shape of target")
        a.labels = _ptr(labels, "labels")
    a.target, a.hist = _ptr(target, "target"), _ptr(hist, "hist")
    for i, m in enumerate(masks):
        a.masks[i] = _ptr(_byte_mask(m, B, S, f"masks[{i}]"), f"masks[{i}]")
    if torch.is_tensor(fov):
        fov = _byte_mask(fov, B, S, "fov")
        a.fov = _ptr(fov, "fov")
    elif fov is not None:
        cam_E, cam_k, origin, voxel_size, img_wh = fov[:5]
        views = tuple(fov[5]) if len(fov) > 5 else (0,)
        if cam_E.dim() != 4 or int(cam_E.shape[0]) != B:
            raise RuntimeError("cam_E must be (batch, views, 4, 4)")
        V = int(cam_E.shape[1])
        _check_calibration(B, V, cam_E, cam_k)
        if not views or any(not 0 <= int(v) < V for v in views):
            raise RuntimeError(f"views must name cameras 0..{V - 1}")
        a.cam_E, a.cam_k = cam_E.data_ptr(), cam_k.data_ptr()
        for j, o in enumerate(origin):
            a.vox_origin[j] = float(o)
        a.voxel_size = float(voxel_size)
        a.n_views, a.img_w, a.img_h = V, int(img_wh[0]), int(img_wh[1])
        a.view_mask = sum({1 << int(v) for v in views})
    for r, (box, need) in enumerate(regions):
        g = a.regions[r]
        g.x0, g.x1, g.y0, g.y1, g.z0, g.z1 = (0, dims[0], 0, dims[1], 0, dims[2]) if box is None else (int(x) for x in box)
        g.need = int(need)
    a.s_b, a.s_c, a.s_v = lay
    a.frame_stride = R * C * C if per_frame else 0
    a.batch, a.C, a.R = B, C, R
    a.X, a.Y, a.Z = dims
    _check(load().occd_ssc_confusion_regions(ctypes.byref(a), _stream()), "occd_ssc_confusion_regions")
    return hist


# ---- relation (context prior) loss, occdepth/loss/CRP_loss.py:4-24 ------------------------------------------------
REL_Q24 = 16777216.0


def _relation_operands(logits, labels):
    if logits.dtype != torch.float32 or not logits.is_cuda or logits.dim() != 4:
        raise RuntimeError("relation logits must be a float32 GPU tensor (B, R, M, N)")
    B, R, M, N = logits.shape
    if labels.dtype not in (torch.uint8, torch.float32, torch.bool) or tuple(labels.shape) != (B, R, N, M) or \
            not labels.is_contiguous() or not labels.is_cuda:
        raise RuntimeError("relation labels must be a contiguous (B, R, N, M) uint8 / bool / float32 GPU tensor")
    st = logits.stride()
    if st[2] != 1 and st[3] != 1:
        raise RuntimeError("relation logits need unit stride along M or N")
    lab = labels.view(torch.uint8) if labels.dtype == torch.bool else labels
    return B, R, M, N, st, lab, (1 if lab.dtype == torch.float32 else 0)


# OCCDEPTH_LOSS_KERNELS=0 restores the ATen formulations of the relation / depth losses and of the frustum-sample backward (A/B)
LOSS_KERNELS = os.environ.get("OCCDEPTH_LOSS_KERNELS", "1") == "1"


def relation_bce_usable(logits, labels):
    """The relation loss runs on `relation_bce_stats` / `relation_bce_grad`: GPU tensors, float logits (B, R, M, N) that are a
    dense permutation with unit stride along M or N, labels (B, R, N, M) uint8 / bool / float32."""
    if not (LOSS_KERNELS and torch.is_tensor(logits) and logits.is_cuda and logits.dim() == 4 and labels.is_cuda):
        return False
    if not (logits.dtype == torch.float32 or (logits.dtype.is_floating_point and torch.is_autocast_enabled())) or \
            labels.dtype not in (torch.uint8, torch.bool, torch.float32):
        return False
    B, R, M, N = logits.shape
    st = logits.stride()
    dense = 1 + sum((n - 1) * s for n, s in zip(logits.shape, st)) == logits.numel()
    return tuple(labels.shape) == (B, R, N, M) and (st[2] == 1 or st[3] == 1) and dense and B * R <= 65535 and R <= 64


def relation_bce_stats(logits, labels):
    """-> int64 (R, 3): #positives, sum_{y=1} softplus(-x) and sum_{y=0} softplus(x) in Q24 (occd_relation_bce_stats)."""
    B, R, M, N, st, lab, ldt = _relation_operands(logits, labels)
    stats = torch.empty((R, 3), dtype=torch.int64, device=logits.device)
    _check(load().occd_relation_bce_stats(logits.data_ptr(), lab.data_ptr(), ldt, stats.data_ptr(), B, R, M, N, st[0], st[1],
                                          st[2], st[3], _stream()), "occd_relation_bce_stats")
    return stats


def relation_bce_grad(logits, labels, coef):
    """d loss / d logits with the logits' strides; coef (R, 2) float32 = g * (pos_weight_r, 1) / (R B M N)."""
    B, R, M, N, st, lab, ldt = _relation_operands(logits, labels)
    if coef.dtype != torch.float32 or tuple(coef.shape) != (R, 2) or not coef.is_contiguous():
        raise RuntimeError("coef must be contiguous float32 (R, 2)")
    dense = sorted(range(4), key=lambda d: -st[d])
    need = 1 + sum((logits.shape[d] - 1) * st[d] for d in range(4))
    if need != logits.numel():
        raise RuntimeError("relation logits must be a dense (permuted) tensor")
    grad = torch.empty_strided(tuple(logits.shape), st, dtype=torch.float32, device=logits.device)
    del dense
    _check(load().occd_relation_bce_grad(logits.data_ptr(), lab.data_ptr(), ldt, coef.data_ptr(), grad.data_ptr(), B, R, M, N,
                                         st[0], st[1], st[2], st[3], _stream()), "occd_relation_bce_grad")
    return grad


# ---- depth-distribution loss, occdepth/loss/depth_loss.py:14-87 ---------------------------------------------------
def depth_bce_usable(preds, labels):
    """The depth loss runs on `depth_bce_stats` / `depth_bce_grad`: float32 GPU predictions and GPU labels."""
    return LOSS_KERNELS and preds.is_cuda and labels.is_cuda and preds.dtype == torch.float32


def _depth_operands(prob, gt, cell):
    if prob.dtype != torch.float32 or not prob.is_cuda or prob.dim() != 4 or not prob[0].is_contiguous():
        raise RuntimeError("depth probabilities must be float32 GPU (Bn, D, h, w) with dense images")
    if gt.dtype != torch.float32 or gt.dim() != 3 or gt.shape[0] != prob.shape[0] or not gt.is_contiguous() or not gt.is_cuda:
        raise RuntimeError("depth labels must be contiguous float32 GPU (Bn, H, W)")
    Bn, D, h, w = prob.shape
    return Bn, D, h, w, gt.shape[1], gt.shape[2], (prob.stride(0) if Bn > 1 else D * h * w)


def depth_bce_stats(prob, gt, cell, d_off, d_step):
    """-> int64 [sum of per-cell BCE over measured cells (Q24), #measured cells] (occd_depth_bce_stats)."""
    Bn, D, h, w, sh, sw, pb = _depth_operands(prob, gt, cell)
    stats = torch.empty(2, dtype=torch.int64, device=prob.device)
    _check(load().occd_depth_bce_stats(prob.data_ptr(), gt.data_ptr(), stats.data_ptr(), Bn, D, h, w, sh, sw, int(cell), pb,
                                       float(d_off), float(d_step), _stream()), "occd_depth_bce_stats")
    return stats


def depth_bce_grad(prob, gt, cell, d_off, d_step, gscale):
    """dense (Bn, D, h, w) d loss / d prob; gscale: one-element float32 device tensor = g / max(1, #measured)."""
    Bn, D, h, w, sh, sw, pb = _depth_operands(prob, gt, cell)
    if gscale.dtype != torch.float32 or gscale.numel() != 1 or not gscale.is_cuda:
        raise RuntimeError("gscale must be a one-element float32 GPU tensor")
    grad = torch.empty((Bn, D, h, w), dtype=torch.float32, device=prob.device)
    _check(load().occd_depth_bce_grad(prob.data_ptr(), gt.data_ptr(), gscale.data_ptr(), grad.data_ptr(), Bn, D, h, w, sh, sw,
                                      int(cell), pb, float(d_off), float(d_step), _stream()), "occd_depth_bce_grad")
    return grad


# ---- depth-rendering loss (K36, csrc/render_loss.hip) ---------------------------------------------------------------
RENDER_LOSS_NORMS = {"abs": RENDER_LOSS_ABS, "rel": RENDER_LOSS_REL}
RENDER_LOSS_MAX_RAYS = 1 << 21           # rays per frame: the bound of the Q32 sums in H
RENDER_LOSS_MAX_DEPTH = 128.0
RENDER_LOSS_MAX_BATCH = 256
RENDER_LOSS_Q32 = 4294967296.0


def render_loss_usable(logits, gt_depth=None):
    """The rendering loss runs on the K36 kernels: float32 GPU logits (B, C, X, Y, Z) with 2 <= C <= 32, and a GPU depth map
    when there is one (a missing library is an error there, as everywhere).  CPU tensors and other dtypes take the torch
    formulation of loss/render_loss.py."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32):
        return False
    if logits.dim() != 5 or not 2 <= logits.shape[1] <= 32 or logits.shape[0] > RENDER_LOSS_MAX_BATCH:
        return False
    return gt_depth is None or gt_depth.is_cuda


def render_loss_rays(image_hw, stride=1, offset=(0, 0)):
    """(h, w) of the ray image: pixel (u, v) = (ou + stride i, ov + stride j), h = ceil((H - ov) / stride), w likewise.
    Raises on a geometry the kernels refuse (no GPU involved)."""
    H, W = int(image_hw[0]), int(image_hw[1])
    s, ou, ov = int(stride), int(offset[0]), int(offset[1])
    if H < 1 or W < 1:
        raise RuntimeError("the depth image must be at least 1 x 1, got %r" % (tuple(image_hw),))
    if s < 1:
        raise RuntimeError("stride must be >= 1, got %r" % (stride,))
    if not (0 <= ou < s and 0 <= ov < s):
        raise RuntimeError("offsets must lie in [0, stride), got %r at stride %d" % (tuple(offset), s))
    if ou >= W or ov >= H:
        raise RuntimeError("offset %r lies outside the %d x %d image" % (tuple(offset), H, W))
    h, w = -(-(H - ov) // s), -(-(W - ou) // s)
    if h * w > RENDER_LOSS_MAX_RAYS:
        raise RuntimeError("%d x %d rays per frame: at most 2^21 (raise the stride)" % (h, w))
    return h, w


def _render_loss_volume(a, logits):
    if not torch.is_tensor(logits) or logits.dtype != torch.float32 or logits.dim() != 5:
        raise RuntimeError("logits must be float32 (B, C, X, Y, Z)")
    B, C, X, Y, Z = (int(d) for d in logits.shape)
    if not 2 <= C <= 32:
        raise RuntimeError("2 <= C <= 32 classes (class 0 is empty), got %d" % C)
    if not 1 <= B <= RENDER_LOSS_MAX_BATCH:
        raise RuntimeError("1 <= B <= %d frames, got %d" % (RENDER_LOSS_MAX_BATCH, B))
    if X * Y * Z >= 1 << 31:
        raise RuntimeError("X Y Z must stay below 2^31")
    a.batch, a.C, a.X, a.Y, a.Z = B, C, X, Y, Z
    return B, C, X * Y * Z


def _render_loss_rays(a, opacity, views, dims, image_hw, stride, offset, max_depth, gt_depth, norm):
    """Fill and check everything the two ray passes share -> (B, h, w)."""
    X, Y, Z = (int(d) for d in dims)
    if min(X, Y, Z) < 1 or X * Y * Z >= 1 << 31:
        raise RuntimeError("dims must be three positive extents with X Y Z < 2^31, got %r" % (tuple(dims),))
    if not torch.is_tensor(opacity) or opacity.dtype != torch.float32 or opacity.dim() != 2 or opacity.shape[1] != X * Y * Z:
        raise RuntimeError("opacity must be float32 (B, X Y Z)")
    B = int(opacity.shape[0])
    if not 1 <= B <= RENDER_LOSS_MAX_BATCH:
        raise RuntimeError("1 <= B <= %d frames, got %d" % (RENDER_LOSS_MAX_BATCH, B))
    if not torch.is_tensor(views) or views.dtype != torch.float32 or tuple(views.shape) != (B, 18):
        raise RuntimeError("views must be float32 (B, 18) with B = %d" % B)
    h, w = render_loss_rays(image_hw, stride, offset)
    md = float(max_depth)
    if not 0.0 < md <= RENDER_LOSS_MAX_DEPTH:
        raise RuntimeError("max_depth must lie in (0, %g], got %r" % (RENDER_LOSS_MAX_DEPTH, max_depth))
    if norm not in RENDER_LOSS_NORMS:
        raise RuntimeError("norm must be 'abs' or 'rel', got %r" % (norm,))
    H, W = int(image_hw[0]), int(image_hw[1])
    if gt_depth is not None:
        if gt_depth.dim() == 4 and gt_depth.shape[1] == 1:
            gt_depth = gt_depth[:, 0]
        if gt_depth.dtype != torch.float32 or tuple(gt_depth.shape) != (B, H, W):
            raise RuntimeError("gt_depth must be float32 (B, 1, H, W) or (B, H, W) with (B, H, W) = %r, got %s %s"
                               % ((B, H, W), tuple(gt_depth.shape), gt_depth.dtype))
        if min(gt_depth.stride()) < 0:
            raise RuntimeError("gt_depth needs non-negative strides")
        if not gt_depth.is_cuda:
            raise RuntimeError("gt_depth must live on the GPU (the HIP kernels have no CPU path)")
        a.gt_depth = gt_depth.data_ptr()
        a.d_b, a.d_h, a.d_w = (int(s) for s in gt_depth.stride())
    a.opacity, a.views = _ptr(opacity, "opacity"), _ptr(views, "views")
    a.batch, a.X, a.Y, a.Z = B, X, Y, Z
    a.H, a.W, a.h, a.w = H, W, h, w
    a.stride, a.off_u, a.off_v = int(stride), int(offset[0]), int(offset[1])
    a.max_depth, a.norm = md, RENDER_LOSS_NORMS[norm]
    return B, h, w


def render_opacity_decode(signed):
    """The opacity a of occd_render_opacity's signed form (a where a <= 1/2, -(1 - a) above, told apart by the sign bit)."""
    return torch.where(torch.signbit(signed), 1.0 + signed, signed)


def render_opacity(logits):
    """occd_render_opacity: a = 1 - softmax(logits)[0] per voxel -> (B, X Y Z) float32 in the signed form the ray passes read
    (`render_opacity_decode`; include/occdepth_amd.h says why).  logits (B, C, X, Y, Z) float32, read in place as planes or
    as channels-last rows (`_logit_layout`); anything else is made contiguous."""
    a = RenderLossArgs()
    B, C, S = _render_loss_volume(a, logits)
    if not logits.is_cuda:
        raise RuntimeError("logits must live on the GPU (the HIP kernels have no CPU path)")
    lay = _logit_layout(logits)
    if lay is None:
        logits = logits.contiguous()
        lay = (C * S, S, 1)
    a.logits = logits.data_ptr()
    a.s_b, a.s_c, a.s_v = lay
    out = torch.empty((B, S), dtype=torch.float32, device=logits.device)
    a.opacity = out.data_ptr()
    _check(load().occd_render_opacity(ctypes.byref(a), _stream()), "occd_render_opacity")
    return out


def render_depth_fwd(opacity, views, dims, image_hw, stride=1, offset=(0, 0), max_depth=RENDER_LOSS_MAX_DEPTH, gt_depth=None,
                     norm="abs"):
    """occd_render_depth_fwd: composite `opacity` (B, X Y Z; `render_opacity`'s signed form or plain values) along the rays of `views` (B, 18) -> (depth (B, h, w), rendered
    opacity (B, h, w), stats).  With gt_depth ((B, 1, H, W) / (B, H, W) float32, read in place through its strides):
    stats = int64 [sum of the per-ray loss (Q24), #valid rays]; without: stats is None.  Contract: include/occdepth_amd.h."""
    a = RenderLossArgs()
    B, h, w = _render_loss_rays(a, opacity, views, dims, image_hw, stride, offset, max_depth, gt_depth, norm)
    depth = torch.empty((B, h, w), dtype=torch.float32, device=opacity.device)
    alpha = torch.empty((B, h, w), dtype=torch.float32, device=opacity.device)
    stats = torch.empty(2, dtype=torch.int64, device=opacity.device) if gt_depth is not None else None
    a.depth, a.alpha = depth.data_ptr(), alpha.data_ptr()
    if stats is not None:
        a.stats = stats.data_ptr()
    _check(load().occd_render_depth_fwd(ctypes.byref(a), _stream()), "occd_render_depth_fwd")
    return depth, alpha, stats


def render_depth_bwd_rays(opacity, views, dims, image_hw, stride, offset, max_depth, gt_depth, norm, depth, hsum):
    """occd_render_depth_bwd_rays: re-walk the valid rays with the forward's `depth` and add every visited voxel's term into
    hsum (B, X Y Z) int64 (Q32; zeroed once by the caller, cleaned by `render_depth_bwd_voxels`) -> hsum."""
    a = RenderLossArgs()
    if gt_depth is None:
        raise RuntimeError("the backward ray pass needs gt_depth")
    B, h, w = _render_loss_rays(a, opacity, views, dims, image_hw, stride, offset, max_depth, gt_depth, norm)
    if not torch.is_tensor(depth) or depth.dtype != torch.float32 or tuple(depth.shape) != (B, h, w):
        raise RuntimeError("depth must be the forward's float32 (B, h, w) = %r image" % ((B, h, w),))
    if not torch.is_tensor(hsum) or hsum.dtype != torch.int64 or tuple(hsum.shape) != tuple(opacity.shape):
        raise RuntimeError("hsum must be int64 of the opacity's shape %r" % (tuple(opacity.shape),))
    a.depth, a.hsum = _ptr(depth, "depth"), _ptr(hsum, "hsum")
    _check(load().occd_render_depth_bwd_rays(ctypes.byref(a), _stream()), "occd_render_depth_bwd_rays")
    return hsum


def render_depth_bwd_voxels(logits, hsum, gscale):
    """occd_render_depth_bwd_voxels: d L / d logits from H, in the logits' layout (channels-last logits get a (B, C, ...) view
    of zero-padded channels-last rows, as `ssc_loss_grad`); hsum is zero afterwards.  gscale: one-element float32 device
    tensor g / max(1, #valid rays)."""
    a = RenderLossArgs()
    B, C, S = _render_loss_volume(a, logits)
    if not torch.is_tensor(hsum) or hsum.dtype != torch.int64 or tuple(hsum.shape) != (B, S):
        raise RuntimeError("hsum must be int64 (B, X Y Z) = %r" % ((B, S),))
    if not torch.is_tensor(gscale) or gscale.dtype != torch.float32 or gscale.numel() != 1:
        raise RuntimeError("gscale must be a one-element float32 GPU tensor")
    if not logits.is_cuda:
        raise RuntimeError("logits must live on the GPU (the HIP kernels have no CPU path)")
    lay = _logit_layout(logits)
    if lay is None:
        logits = logits.contiguous()
        lay = (C * S, S, 1)
    if lay[1] == 1:
        cs = round_up(C, 8)
        rows = torch.empty((B,) + tuple(logits.shape[2:]) + (cs,), dtype=torch.float32, device=logits.device)
        grad = rows[..., :C].permute(0, 4, 1, 2, 3)
        glay, gpad = (S * cs, 1, cs), cs
    else:
        grad = torch.empty_like(logits)
        glay, gpad = lay, 0
    a.logits, a.grad = logits.data_ptr(), grad.data_ptr()
    a.hsum, a.gscale = _ptr(hsum, "hsum"), _ptr(gscale, "gscale")
    a.s_b, a.s_c, a.s_v = lay
    a.g_b, a.g_c, a.g_v = glay
    a.g_pad = gpad
    _check(load().occd_render_depth_bwd_voxels(ctypes.byref(a), _stream()), "occd_render_depth_bwd_voxels")
    return grad


# ---- stable segmented radix sort (K38, csrc/sort.hip) ----------------------------------------------------------------
def sort_passes(begin_bit=0, end_bit=32):
    """Passes of `sort_pairs` over key bits [begin_bit, end_bit); the result lands in buffer passes % 2."""
    if not 0 <= int(begin_bit) < int(end_bit) <= 32:
        raise ValueError("the bit range must be 0 <= begin_bit < end_bit <= 32, got [%r, %r)" % (begin_bit, end_bit))
    return -(-(int(end_bit) - int(begin_bit)) // SORT_RADIX_BITS)


def sort_hist_words(segments, n):
    """uint32 words of the histogram workspace `sort_pairs` needs for (segments, n)."""
    return int(segments) * (1 << SORT_RADIX_BITS) * (-(-int(n) // SORT_TILE))


def sort_scratch(segments, n, device):
    """(keys_alt, vals_alt, hist) for `sort_pairs` of (segments, n) pairs."""
    alt = torch.empty((2, int(segments), int(n)), dtype=torch.int32, device=device)
    return alt[0], alt[1], torch.empty(sort_hist_words(segments, n), dtype=torch.int32, device=device)


def sort_pairs(keys, vals, begin_bit=0, end_bit=32, scratch=None):
    """occd_sort_pairs_u32: sort every row of keys (S, n) -- int32 tensors read as uint32 -- ascending on key bits
    [begin_bit, end_bit), stably, carrying vals (S, n) -> (sorted keys, sorted vals).  `keys` and `vals` are OVERWRITTEN
    (they are one of the two ping-pong buffers); the returned tensors are either they or the scratch's, whichever the
    last pass wrote.  scratch: `sort_scratch(S, n, device)`, made here when None.  No host read: capture-safe when the
    scratch is given."""
    for t, name in ((keys, "keys"), (vals, "vals")):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 2:
            raise RuntimeError("%s must be int32 (S, n) (the bits of uint32 values)" % name)
    if keys.shape != vals.shape:
        raise RuntimeError("keys %s and vals %s differ in shape" % (tuple(keys.shape), tuple(vals.shape)))
    S, n = (int(d) for d in keys.shape)
    if n < 1 or n >= 1 << 31 or not 1 <= S <= 65535:
        raise RuntimeError("sort_pairs needs 1 <= n < 2^31 and 1 <= S <= 65535, got (S, n) = (%d, %d)" % (S, n))
    passes = sort_passes(begin_bit, end_bit)
    if scratch is None:
        scratch = sort_scratch(S, n, keys.device)
    kalt, valt, hist = scratch
    if tuple(kalt.shape) != (S, n) or tuple(valt.shape) != (S, n) or kalt.dtype != torch.int32 or valt.dtype != torch.int32:
        raise RuntimeError("the scratch pair buffers must be int32 (S, n) = %r" % ((S, n),))
    if hist.dtype != torch.int32 or hist.numel() < sort_hist_words(S, n):
        raise RuntimeError("the scratch histogram needs %d int32 words" % sort_hist_words(S, n))
    a = SortArgs()
    a.keys, a.vals = _ptr(keys, "keys"), _ptr(vals, "vals")
    a.keys_alt, a.vals_alt, a.hist = _ptr(kalt, "keys_alt"), _ptr(valt, "vals_alt"), _ptr(hist, "hist")
    a.n, a.segments, a.begin_bit, a.end_bit = n, S, int(begin_bit), int(end_bit)
    _check(load().occd_sort_pairs_u32(ctypes.byref(a), _stream()), "occd_sort_pairs_u32")
    return (kalt, valt) if passes & 1 else (keys, vals)


# ---- surface mesh of a brick volume (K39, csrc/mesh.hip, welded on K38) ----------------------------------------------
MESH_MAX_CORNERS = (1 << 31) - 1         # 4 F corner references are one segment of sort_pairs


def mesh_key_bits(grid):
    """(bx, by, bz): the bits of a lattice corner's coordinates in the key x << (by + bz) | y << bz | z of a window of
    `grid` = (gx, gy, gz) bricks, b = bit_length(16 g).  ValueError for a window over the directory's limits."""
    grid = tuple(int(g) for g in grid)
    if len(grid) != 3 or min(grid) < 1 or max(grid) > MESH_MAX_GRID or grid[0] * grid[1] * grid[2] > MESH_MAX_CELLS:
        raise ValueError("the window is %s bricks: 1 .. 2^16 along an axis and at most 2^27 cells can be meshed; take a part "
                         "of the map with key_range" % (grid,))
    return tuple((MAP_BRICK * g).bit_length() for g in grid)


def _mesh_volume_args(labels, cells, cap_unknown=True, cells_host=None):
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 2 or labels.shape[0] < 1 or \
            labels.shape[1] != _MAP_BRICK_VOX:
        raise RuntimeError("labels must be uint8 (n, %d) brick rows" % _MAP_BRICK_VOX)
    if not torch.is_tensor(cells) or cells.dtype != torch.int32 or cells.dim() != 3 or cells.device != labels.device:
        raise RuntimeError("cells must be an int32 (gx, gy, gz) directory on the device of labels")
    mesh_key_bits(cells.shape)
    a = MeshArgs()
    a.labels, a.cells = _ptr(labels, "labels"), _ptr(cells, "cells")
    if cells_host is not None:
        if cells_host.is_cuda or cells_host.dtype != torch.int32 or cells_host.shape != cells.shape or not cells_host.is_contiguous():
            raise RuntimeError("cells_host must be the directory's contiguous int32 copy in host memory")
        a.cells_host = cells_host.data_ptr()
    a.gx, a.gy, a.gz = (int(d) for d in cells.shape)
    a.n_rows, a.cap_unknown = int(labels.shape[0]), int(bool(cap_unknown))
    return a


def mesh_count(labels, cells, cap_unknown=True, cells_host=None):
    """occd_mesh_count: -> (counts (n,) int32, the faces of every brick row; row_cell (n,) int32, the workspace
    `mesh_emit` reads).  labels (n, 4096) uint8 brick rows, cells (gx, gy, gz) int32 directory (semantic_map.MapVolume)."""
    a = _mesh_volume_args(labels, cells, cap_unknown, cells_host)
    n = int(labels.shape[0])
    counts = torch.empty((n,), dtype=torch.int32, device=labels.device)
    row_cell = torch.empty((n,), dtype=torch.int32, device=labels.device)
    a.counts, a.row_cell = counts.data_ptr(), row_cell.data_ptr()
    _check(load().occd_mesh_count(ctypes.byref(a), _stream()), "occd_mesh_count")
    return counts, row_cell


def mesh_emit(labels, cells, row_cell, offsets, n_faces, cap_unknown=True, cells_host=None):
    """occd_mesh_emit: the faces behind `offsets` (n,) int64, the exclusive scan of mesh_count's counts -> face_label (F,),
    face_dir (F,) uint8 and the 4 F corner references keys_lo, keys_hi (None for a key of at most 32 bits), refs, int32
    tensors holding uint32 bits."""
    a = _mesh_volume_args(labels, cells, cap_unknown, cells_host)
    F, dev = int(n_faces), labels.device
    face_label = torch.empty((F,), dtype=torch.uint8, device=dev)
    face_dir = torch.empty((F,), dtype=torch.uint8, device=dev)
    keys_lo = torch.empty((4 * F,), dtype=torch.int32, device=dev)
    keys_hi = torch.empty((4 * F,), dtype=torch.int32, device=dev) if sum(mesh_key_bits(cells.shape)) > 32 else None
    refs = torch.empty((4 * F,), dtype=torch.int32, device=dev)
    if offsets.dtype != torch.int64 or offsets.numel() != labels.shape[0] or row_cell.dtype != torch.int32 or \
            row_cell.numel() != labels.shape[0]:
        raise RuntimeError("offsets must be int64 (n,) and row_cell int32 (n,)")
    a.row_cell, a.offsets = _ptr(row_cell, "row_cell"), _ptr(offsets, "offsets")
    a.face_label, a.face_dir, a.keys_lo, a.refs = face_label.data_ptr(), face_dir.data_ptr(), keys_lo.data_ptr(), refs.data_ptr()
    a.keys_hi = None if keys_hi is None else keys_hi.data_ptr()
    a.n_faces = F
    _check(load().occd_mesh_emit(ctypes.byref(a), _stream()), "occd_mesh_emit")
    return face_label, face_dir, keys_lo, keys_hi, refs


def _mesh_corner_args(keys_lo, keys_hi, grid):
    n = int(keys_lo.numel())
    if keys_lo.dtype != torch.int32 or n < 4 or n % 4 or (keys_hi is not None and (keys_hi.dtype != torch.int32 or keys_hi.numel() != n)):
        raise RuntimeError("the sorted keys must be int32 (4 F,) tensors (the bits of uint32 values)")
    if sum(mesh_key_bits(grid)) > 32 and keys_hi is None:
        raise RuntimeError("a window of %s bricks has keys of more than 32 bits: the high words are missing" % (tuple(grid),))
    a = MeshArgs()
    a.gx, a.gy, a.gz = (int(g) for g in grid)
    a.n_rows, a.n_faces = 1, n // 4
    a.keys_lo, a.keys_hi = _ptr(keys_lo, "keys_lo"), _ptr(keys_hi, "keys_hi")
    return a, n


def mesh_heads(keys_lo, keys_hi, grid):
    """occd_mesh_heads on the SORTED keys -> marks (4 F,) int32, 1 where a key differs from its predecessor's."""
    a, n = _mesh_corner_args(keys_lo, keys_hi, grid)
    marks = torch.empty((n,), dtype=torch.int32, device=keys_lo.device)
    a.marks = marks.data_ptr()
    _check(load().occd_mesh_heads(ctypes.byref(a), _stream()), "occd_mesh_heads")
    return marks


def mesh_weld(keys_lo, keys_hi, refs, ranks, n_vertices, grid):
    """occd_mesh_weld on the sorted (key, ref) pairs and `ranks`, the inclusive int32 scan of mesh_heads' marks ->
    quads (F, 4) int32, vertices (V, 3) int32."""
    a, n = _mesh_corner_args(keys_lo, keys_hi, grid)
    if refs.dtype != torch.int32 or refs.numel() != n or ranks.dtype != torch.int32 or ranks.numel() != n:
        raise RuntimeError("refs and ranks must be int32 (4 F,) tensors")
    V = int(n_vertices)
    quads = torch.empty((n // 4, 4), dtype=torch.int32, device=keys_lo.device)
    vertices = torch.empty((V, 3), dtype=torch.int32, device=keys_lo.device)
    a.refs, a.ranks, a.quads, a.vertices, a.n_vertices = _ptr(refs, "refs"), _ptr(ranks, "ranks"), quads.data_ptr(), vertices.data_ptr(), V
    _check(load().occd_mesh_weld(ctypes.byref(a), _stream()), "occd_mesh_weld")
    return quads, vertices


def mesh_sort_corners(keys_lo, keys_hi, refs, bits):
    """The (key, ref) pairs ascending in the key, stably, on exactly its `bits` bits: one sort_pairs for a key of at most
    32 bits; else the low word first, the high words gathered by that permutation and sorted next (K38 is stable, so the two
    are an LSD sort of the two-word key) -> (keys_lo, keys_hi, refs), sorted."""
    n = int(keys_lo.numel())
    if bits <= 32:
        lo, ref = sort_pairs(keys_lo.view(1, n), refs.view(1, n), 0, bits)
        return lo.reshape(n), None, ref.reshape(n)
    lo0 = keys_lo.clone()                                              # sort_pairs overwrites its input
    _, ref = sort_pairs(keys_lo.view(1, n), refs.view(1, n), 0, 32)
    hi = keys_hi[ref.reshape(n).long()]
    hi, ref = sort_pairs(hi.view(1, n), ref.reshape(1, n).contiguous(), 0, bits - 32)
    ref = ref.reshape(n)
    return lo0[ref.long()], hi.reshape(n), ref


def mesh_faces(labels, cells, cap_unknown=True, cells_host=None):
    """The indexed quad mesh of a brick volume (K39; the contract is in include/occdepth_amd.h): occd_mesh_count ->
    exclusive scan -> occd_mesh_emit -> sort_pairs (K38) over the key's bits -> occd_mesh_heads -> inclusive scan ->
    occd_mesh_weld.  labels (n, 4096) uint8 brick rows, cells (gx, gy, gz) int32 -> vertices (V, 3) int32 lattice corners
    ascending in (x, y, z), quads (F, 4) int32, face_label (F,) uint8, face_dir (F,) uint8, faces ascending in (row, voxel,
    face code).  Two host synchronisations, for F and for V; a volume without a face launches nothing after the count."""
    bits = sum(mesh_key_bits(cells.shape))
    counts, row_cell = mesh_count(labels, cells, cap_unknown, cells_host)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    F = int(ends[-1])
    dev = labels.device
    if 4 * F > MESH_MAX_CORNERS:
        raise ValueError("the volume has %d faces: 4 F = %d corner references are more than the 2^31 - 1 one sort takes; "
                         "mesh a part of the map with key_range" % (F, 4 * F))
    if F == 0:
        return (torch.empty((0, 3), dtype=torch.int32, device=dev), torch.empty((0, 4), dtype=torch.int32, device=dev),
                torch.empty((0,), dtype=torch.uint8, device=dev), torch.empty((0,), dtype=torch.uint8, device=dev))
    offsets = (ends - counts).contiguous()
    face_label, face_dir, keys_lo, keys_hi, refs = mesh_emit(labels, cells, row_cell, offsets, F, cap_unknown, cells_host)
    keys_lo, keys_hi, refs = mesh_sort_corners(keys_lo, keys_hi, refs, bits)
    ranks = torch.cumsum(mesh_heads(keys_lo, keys_hi, cells.shape), 0, dtype=torch.int32)
    quads, vertices = mesh_weld(keys_lo, keys_hi, refs, ranks, int(ranks[-1]), cells.shape)
    return vertices, quads, face_label, face_dir


# ---- connected components of a label volume (K40, csrc/ccl.hip; the overlaps are sorted on K38) ----------------------
def ccl_class_mask(classes):
    """The 256-bit class mask of the C ABI (8 uint32 words, bit l of word l >> 5) of an iterable of labels 0..255."""
    words = [0] * 8
    for c in classes or ():
        c = int(c)
        if not 0 <= c <= 255:
            raise ValueError("a class must be 0..255, got %r" % (c,))
        words[c >> 5] |= 1 << (c & 31)
    return tuple(words)


def ccl_workspace(batch, dims, device):
    """(parent (B, N) int32, stuff_min (B, 256) int32, status (1,) int32): the workspace of `ccl_segments` and `ccl_filter`
    for `batch` frames of `dims` = (X, Y, Z): 4 B N + 1024 B + 4 bytes."""
    n = int(dims[0]) * int(dims[1]) * int(dims[2])
    return (torch.empty((int(batch), n), dtype=torch.int32, device=device),
            torch.empty((int(batch), 256), dtype=torch.int32, device=device), torch.zeros((1,), dtype=torch.int32, device=device))


def _ccl_volume_args(labels, things, stuff, name="labels"):
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 4 or labels.numel() == 0:
        raise RuntimeError("%s must be a non-empty uint8 (B, X, Y, Z) tensor" % name)
    B, X, Y, Z = (int(d) for d in labels.shape)
    if X * Y * Z >= (1 << 31) - 1 or B > 65535:
        raise ValueError("a frame of %d voxels (B = %d): a frame must stay below 2^31 - 1 voxels and B below 65536" % (X * Y * Z, B))
    a = CclArgs()
    a.batch, a.X, a.Y, a.Z = B, X, Y, Z
    t, s = ccl_class_mask(things), ccl_class_mask(stuff)
    if any(x & y for x, y in zip(t, s)):
        raise ValueError("things %r and stuff %r overlap" % (sorted(things), sorted(stuff)))
    a.things[:], a.stuff[:] = t, s
    a.labels = _ptr(labels, name)
    return a


def _ccl_check_workspace(workspace, labels):
    B, n = int(labels.shape[0]), int(labels[0].numel())
    if workspace is None:
        workspace = ccl_workspace(B, labels.shape[1:], labels.device)
    parent, stuff_min, status = workspace
    for t, need, name in ((parent, B * n, "parent"), (stuff_min, B * 256, "stuff_min"), (status, 1, "status")):
        if t.dtype != torch.int32 or t.numel() < need or t.device != labels.device:
            raise RuntimeError("the workspace's %s must be int32 of at least %d elements on the device of labels" % (name, need))
    return workspace


def ccl_status(workspace):
    """Read the status word `ccl_segments` left in its workspace (one host synchronisation) and raise on a set bit."""
    code = int(workspace[2][0])
    if code & CCL_STATUS_OVERRUN:
        raise RuntimeError("occd_ccl_segments: a bounded union-find loop ran out (status %d): a bug or a corrupted workspace" % code)
    if code & CCL_STATUS_INSTANCE:
        raise ValueError("occd_ccl_segments: an instance id carries voxels of more than one class (status %d)" % code)


def ccl_segments(labels, things, stuff=(), connectivity=26, workspace=None, instances=None, tile_pass=True, check=True):
    """occd_ccl_segments: labels (B, X, Y, Z) uint8 -> seg (B, X, Y, Z) int32, 0 outside every segment, else 1 + the smallest
    frame-linear index of the voxel's segment (the contract is in include/occdepth_amd.h).  things / stuff: iterables of
    classes; instances (B, X, Y, Z) int32: the things segments are the instance ids 1 .. N - 1 instead of the components.
    workspace: `ccl_workspace(...)`, made here when None.  check: read the status word (one host synchronisation) and
    raise if a kernel set it; with check=False nothing is read -- call `ccl_status(workspace)` later.
    tile_pass=False runs the seam pass over every voxel pair (the same result; for measurements)."""
    if int(connectivity) not in (6, 26):
        raise ValueError("connectivity must be 6 or 26, got %r" % (connectivity,))
    a = _ccl_volume_args(labels, things, stuff)
    workspace = _ccl_check_workspace(workspace, labels)
    seg = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    if instances is not None:
        if not torch.is_tensor(instances) or instances.dtype != torch.int32 or instances.shape != labels.shape:
            raise RuntimeError("instances must be an int32 tensor of labels' shape")
        a.instances = _ptr(instances, "instances")
    a.parent, a.stuff_min, a.status = (_ptr(t, "workspace") for t in workspace)
    a.seg, a.connectivity, a.flags = seg.data_ptr(), int(connectivity), 0 if tile_pass else CCL_NO_TILE_PASS
    _check(load().occd_ccl_segments(ctypes.byref(a), _stream()), "occd_ccl_segments")
    if check:
        ccl_status(workspace)
    return seg


def ccl_compact(seg, labels):
    """Number the segments of every frame 1 .. K_b in ascending order of seg: occd_ccl_roots -> a scan within each frame ->
    occd_ccl_compact.  -> ids (B, X, Y, Z) int32 (0 kept), count (B,) int64 (a HOST tensor: the one host read), offsets (B,)
    int64 on the device (the exclusive scan of count) and the tables of sum(count) rows, frame after frame: seg_class
    uint8, seg_size int32 (voxels), seg_index int32 (the smallest voxel index, seg - 1)."""
    if not torch.is_tensor(seg) or seg.dtype != torch.int32 or seg.shape != labels.shape:
        raise RuntimeError("seg must be the int32 tensor ccl_segments made of labels")
    a = _ccl_volume_args(labels, (), ())
    B, n, dev = int(labels.shape[0]), int(labels[0].numel()), labels.device
    marks = torch.empty((B, n), dtype=torch.int32, device=dev)
    a.seg, a.marks = _ptr(seg, "seg"), marks.data_ptr()
    _check(load().occd_ccl_roots(ctypes.byref(a), _stream()), "occd_ccl_roots")
    ranks = torch.cumsum(marks, 1, dtype=torch.int32)
    count_dev = ranks[:, -1].to(torch.int64)
    offsets = (torch.cumsum(count_dev, 0) - count_dev).contiguous()
    count = count_dev.cpu()
    K = int(count.sum())
    ids = torch.empty(labels.shape, dtype=torch.int32, device=dev)
    seg_class = torch.empty((K,), dtype=torch.uint8, device=dev)
    seg_size = torch.empty((K,), dtype=torch.int32, device=dev)
    seg_index = torch.empty((K,), dtype=torch.int32, device=dev)
    a.ranks, a.offsets, a.ids, a.n_segments = _ptr(ranks, "ranks"), _ptr(offsets, "offsets"), ids.data_ptr(), K
    if K:
        a.seg_class, a.seg_size, a.seg_index = seg_class.data_ptr(), seg_size.data_ptr(), seg_index.data_ptr()
    _check(load().occd_ccl_compact(ctypes.byref(a), _stream()), "occd_ccl_compact")
    return ids, count, offsets, (seg_class, seg_size, seg_index)


def ccl_filter(labels, things, min_voxels, connectivity=26, stuff=(), workspace=None, seg=None, check=True):
    """occd_ccl_filter: a copy of labels (B, X, Y, Z) uint8 in which every voxel of a things segment of fewer than
    min_voxels voxels is 0 (stuff and all other voxels pass).  seg: `ccl_segments(labels, things, stuff, connectivity)`
    when the caller has it; else it is made here, in the same workspace."""
    if not 1 <= int(min_voxels) <= (1 << 31) - 1:
        raise ValueError("min_voxels must be 1 .. 2^31 - 1, got %r" % (min_voxels,))
    a = _ccl_volume_args(labels, things, stuff)
    workspace = _ccl_check_workspace(workspace, labels)
    if seg is None:
        seg = ccl_segments(labels, things, stuff, connectivity, workspace, check=check)
    elif seg.dtype != torch.int32 or seg.shape != labels.shape:
        raise RuntimeError("seg must be the int32 tensor ccl_segments made of labels")
    out = torch.empty_like(labels)
    a.seg, a.parent, a.out, a.min_voxels = _ptr(seg, "seg"), _ptr(workspace[0], "workspace"), out.data_ptr(), int(min_voxels)
    _check(load().occd_ccl_filter(ctypes.byref(a), _stream()), "occd_ccl_filter")
    return out


def ccl_sort_pairs(keys_lo, keys_hi, refs, lo_bits, hi_bits):
    """The emitted (key, ref) pairs ascending in the key, stably, over exactly its bits: one `sort_pairs` over lo_bits +
    hi_bits for a one-word key (keys_hi None); else keys_lo over lo_bits first, the high words gathered by that
    permutation and sorted over hi_bits next (K38 is stable, so the two stages are an LSD sort of the two-word key) ->
    (keys_lo, keys_hi), sorted."""
    n = int(keys_lo.numel())
    if keys_hi is None:
        lo, _ = sort_pairs(keys_lo.view(1, n), refs.view(1, n), 0, lo_bits + hi_bits)
        return lo.reshape(n), None
    lo0 = keys_lo.clone()                                              # sort_pairs overwrites its input
    _, ref = sort_pairs(keys_lo.view(1, n), refs.view(1, n), 0, lo_bits)
    hi = keys_hi[ref.reshape(n).long()]
    hi, ref = sort_pairs(hi.view(1, n), ref.reshape(1, n).contiguous(), 0, hi_bits)
    return lo0[ref.reshape(n).long()], hi.reshape(n)


def ccl_overlaps(g_ids, g_count, g_offsets, p_ids, p_count, p_offsets, target, mask=None):
    """The exact overlap counts of two compacted segment volumes of the same frames (occd_ccl_pair_*; the contract is in
    include/occdepth_amd.h): g_ids / p_ids, count (host) and offsets as `ccl_compact` returns them for the target and the
    prediction; target (B, X, Y, Z) uint8 (255 = not valid), mask None or uint8 / bool of the same shape.  -> rows (R, 3)
    int32 on the device: (g, p, n) with g, p the GLOBAL ids (offsets[b] + id, 0 = no segment), ascending in (g, p), n the
    valid voxels that carry the pair.  Two host reads (the pairs, the rows)."""
    B, n, dev = int(g_ids.shape[0]), int(g_ids[0].numel()), g_ids.device
    for t, name in ((g_ids, "g_ids"), (p_ids, "p_ids")):
        if t.dtype != torch.int32 or t.shape != g_ids.shape:
            raise RuntimeError("%s must be int32 (B, X, Y, Z)" % name)
    if target.dtype != torch.uint8 or target.numel() != g_ids.numel():
        raise RuntimeError("target must be uint8 of the ids' size")
    if B * n >= 1 << 31:
        raise ValueError("%d voxels in the batch: the overlaps of one call take fewer than 2^31" % (B * n))
    a = CclPairArgs()
    a.g_ids, a.p_ids, a.target = _ptr(g_ids, "g_ids"), _ptr(p_ids, "p_ids"), _ptr(target, "target")
    if mask is not None:
        if mask.dtype == torch.bool:
            mask = mask.to(torch.uint8)
        if mask.dtype != torch.uint8 or mask.numel() != g_ids.numel():
            raise RuntimeError("mask must be bool / uint8 of the ids' size")
        a.mask = _ptr(mask, "mask")
    g_bits, p_bits = max(1, int(g_count.sum()).bit_length()), max(1, int(p_count.sum()).bit_length())
    a.n, a.batch, a.p_bits = n, B, p_bits
    marks = torch.empty((B * n,), dtype=torch.int32, device=dev)
    a.marks = marks.data_ptr()
    _check(load().occd_ccl_pair_marks(ctypes.byref(a), _stream()), "occd_ccl_pair_marks")
    pos = torch.cumsum(marks, 0, dtype=torch.int32)
    P = int(pos[-1])
    if P == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=dev)
    keys_lo = torch.empty((P,), dtype=torch.int32, device=dev)
    keys_hi = torch.empty((P,), dtype=torch.int32, device=dev) if g_bits + p_bits > 32 else None
    refs = torch.empty((P,), dtype=torch.int32, device=dev)
    a.pos, a.g_offsets, a.p_offsets = _ptr(pos, "pos"), _ptr(g_offsets, "g_offsets"), _ptr(p_offsets, "p_offsets")
    a.keys_lo, a.keys_hi, a.refs, a.n_pairs = keys_lo.data_ptr(), _ptr(keys_hi, "keys_hi"), refs.data_ptr(), P
    _check(load().occd_ccl_pair_emit(ctypes.byref(a), _stream()), "occd_ccl_pair_emit")
    keys_lo, keys_hi = ccl_sort_pairs(keys_lo, keys_hi, refs, p_bits, g_bits)
    heads = torch.empty((P,), dtype=torch.int32, device=dev)
    a.keys_lo, a.keys_hi, a.marks = _ptr(keys_lo, "keys_lo"), _ptr(keys_hi, "keys_hi"), heads.data_ptr()
    _check(load().occd_ccl_pair_heads(ctypes.byref(a), _stream()), "occd_ccl_pair_heads")
    ranks = torch.cumsum(heads, 0, dtype=torch.int32)
    R = int(ranks[-1])
    rows = torch.empty((4, R), dtype=torch.int32, device=dev)
    a.ranks, a.n_rows = _ptr(ranks, "ranks"), R
    a.row_start, a.row_g, a.row_p, a.row_n = (rows[i].data_ptr() for i in range(4))
    _check(load().occd_ccl_pair_rows(ctypes.byref(a), _stream()), "occd_ccl_pair_rows")
    return rows[1:].t().contiguous()


# ---- Lovasz-softmax loss (csrc/lovasz.hip, on K38) -------------------------------------------------------------------
LOVASZ_MAX_VOXELS = (1 << 31) - 1        # the payload keeps the voxel index in 31 bits, the fg flag in bit 31
LOVASZ_ONE_BITS = 0x3F800000


def lovasz_usable(logits, target=None):
    """The Lovasz-softmax loss runs on the K38 kernels: float32 GPU logits (B, C, ...) with 2 <= C <= 32 and a GPU uint8
    target (a missing library is an error there, as everywhere).  CPU tensors and other dtypes take the torch formulation
    of loss/lovasz_loss.py."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32):
        return False
    if logits.dim() < 3 or not 2 <= logits.shape[1] <= 32:
        return False
    return target is None or (target.is_cuda and target.dtype == torch.uint8)


def lovasz_check_voxels(n):
    """N = B X Y Z voxels must leave bit 31 of the sort payload to the fg flag."""
    if int(n) < 1 or int(n) > LOVASZ_MAX_VOXELS:
        raise ValueError("the Lovasz-softmax loss takes 1 <= N < 2^31 voxels per call, got %d" % int(n))
    return int(n)


def lovasz_value_bound(n):
    """Worst-case rounding of a class loss L_c against exact arithmetic on the same float32 errors
    (include/occdepth_amd.h): half a Q60 unit per voxel + the float64 roundings of g, e g and the scaling."""
    return int(n) * 2.0 ** -(LOVASZ_Q + 1) + 2.0 ** -50


def lovasz_chunk(n_classes, class_chunk=None):
    cc = int(n_classes) if class_chunk is None else int(class_chunk)
    if not 1 <= cc <= int(n_classes):
        raise ValueError("class_chunk must lie in 1 .. C = %d, got %r" % (n_classes, class_chunk))
    return cc


def lovasz_scratch_bytes(n, n_classes, class_chunk=None):
    """Bytes of cached scratch the loss holds for N voxels and C classes sorted `class_chunk` at a time: two ping-pong
    buffers of (key, value) pairs, the sort's histograms and the tile sums of the ranks pass.  (The table q, N C floats,
    is the forward's saved state, not scratch.)"""
    n, cc = lovasz_check_voxels(n), lovasz_chunk(n_classes, class_chunk)
    return 16 * cc * n + 4 * sort_hist_words(cc, n) + 4 * cc * (-(-n // LOVASZ_RANK_TILE))


_lovasz_scratch = {}


def lovasz_scratch(n, cc, device):
    """The cached scratch of one (N, classes per group, device): {"pairs": int32 (2, 2, cc, N), "hist", "tsum"}."""
    key = (int(n), int(cc), str(device))
    sc = _lovasz_scratch.get(key)
    if sc is None:
        sc = _lovasz_scratch[key] = {
            "pairs": torch.empty((2, 2, cc, n), dtype=torch.int32, device=device),
            "hist": torch.empty(sort_hist_words(cc, n), dtype=torch.int32, device=device),
            "tsum": torch.empty(cc * (-(-n // LOVASZ_RANK_TILE)), dtype=torch.int32, device=device)}
    return sc


def _lovasz_logits(a, logits, target, ignore):
    if not torch.is_tensor(logits) or logits.dtype != torch.float32 or logits.dim() < 3:
        raise RuntimeError("logits must be float32 (B, C, ...)")
    if not logits.is_cuda:
        raise RuntimeError("logits must live on the GPU (the HIP kernels have no CPU path)")
    B, C = int(logits.shape[0]), int(logits.shape[1])
    S = logits[0, 0].numel()
    if not 2 <= C <= 32:
        raise RuntimeError("2 <= C <= 32 classes, got %d" % C)
    lovasz_check_voxels(B * S)
    if target.dtype != torch.uint8 or tuple(target.shape) != (B,) + tuple(logits.shape[2:]):
        raise RuntimeError("target must be uint8 of shape (B, ...) = %r" % ((B,) + tuple(logits.shape[2:]),))
    lay = _logit_layout(logits)
    if lay is None:
        logits = logits.contiguous()
        lay = (C * S, S, 1)
    target = target.contiguous()
    a.logits, a.target = logits.data_ptr(), _ptr(target, "target")
    a.s_b, a.s_c, a.s_v = lay
    a.batch, a.C, a.S, a.ignore = B, C, S, int(ignore)
    return logits, target, lay, B, C, S


def lovasz_errors(logits, target, c0, cc, keys, vals, ignore=255):
    """occd_lovasz_errors: softmax per voxel; for the classes c0 .. c0 + cc - 1 the sort key (LOVASZ_ONE_BITS - bits(e):
    ascending key = descending error; LOVASZ_INVALID_KEY where target == ignore) and the payload (voxel | fg << 31) into
    keys, vals (cc, N) int32."""
    a = LovaszArgs()
    keep = _lovasz_logits(a, logits, target, ignore)
    N = keep[3] * keep[5]
    for t, name in ((keys, "keys"), (vals, "vals")):
        if t.dtype != torch.int32 or tuple(t.shape) != (int(cc), N):
            raise RuntimeError("%s must be int32 (cc, N) = %r" % (name, (int(cc), N)))
    a.c0, a.cc = int(c0), int(cc)
    a.keys, a.vals = _ptr(keys, "keys"), _ptr(vals, "vals")
    _check(load().occd_lovasz_errors(ctypes.byref(a), _stream()), "occd_lovasz_errors")
    return keys, vals


def lovasz_ranks(keys, vals, c0, q, fg_count, loss_q, tsum=None):
    """occd_lovasz_ranks on SORTED keys, vals (cc, N): writes q[:, c0:c0 + cc] (q is (N, C) float32: the signed Jaccard
    increment of every valid voxel), fg_count[c0:c0 + cc] (G_c) and loss_q[c0:c0 + cc] (L_c in Q60), both int64 (C,)."""
    cc, N = (int(d) for d in keys.shape)
    lovasz_check_voxels(N)
    if keys.dtype != torch.int32 or vals.dtype != torch.int32 or tuple(vals.shape) != (cc, N):
        raise RuntimeError("keys and vals must be int32 (cc, N)")
    if q.dtype != torch.float32 or q.dim() != 2 or q.shape[0] != N or not 2 <= q.shape[1] <= 32:
        raise RuntimeError("q must be float32 (N, C) with N = %d and 2 <= C <= 32" % N)
    C = int(q.shape[1])
    if not (0 <= int(c0) and int(c0) + cc <= C):
        raise RuntimeError("classes %d .. %d lie outside 0 .. %d" % (c0, int(c0) + cc - 1, C - 1))
    for t, name in ((fg_count, "fg_count"), (loss_q, "loss_q")):
        if t.dtype != torch.int64 or tuple(t.shape) != (C,):
            raise RuntimeError("%s must be int64 (C,) = (%d,)" % (name, C))
    words = cc * (-(-N // LOVASZ_RANK_TILE))
    if tsum is None:
        tsum = torch.empty(words, dtype=torch.int32, device=keys.device)
    if tsum.dtype != torch.int32 or tsum.numel() < words:
        raise RuntimeError("tsum needs %d int32 words" % words)
    a = LovaszArgs()
    a.keys, a.vals, a.tsum, a.q = _ptr(keys, "keys"), _ptr(vals, "vals"), _ptr(tsum, "tsum"), _ptr(q, "q")
    a.fg_count, a.loss_q = _ptr(fg_count, "fg_count"), _ptr(loss_q, "loss_q")
    a.batch, a.S, a.C, a.c0, a.cc = 1, N, C, int(c0), cc
    _check(load().occd_lovasz_ranks(ctypes.byref(a), _stream()), "occd_lovasz_ranks")
    return q, fg_count, loss_q


def lovasz_bwd(logits, target, q, gscale, ignore=255):
    """occd_lovasz_bwd: d L / d logits = gscale p_j (q_j - sum_c q_c p_c) per voxel, zeros where target == ignore, in the
    logits' layout (channels-last logits get a (B, C, ...) view of zero-padded channels-last rows, as `ssc_loss_grad`).
    gscale: one-element float32 device tensor (incoming gradient / #present)."""
    a = LovaszArgs()
    logits, target, lay, B, C, S = _lovasz_logits(a, logits, target, ignore)
    if q.dtype != torch.float32 or tuple(q.shape) != (B * S, C):
        raise RuntimeError("q must be float32 (N, C) = %r" % ((B * S, C),))
    if not torch.is_tensor(gscale) or gscale.dtype != torch.float32 or gscale.numel() != 1:
        raise RuntimeError("gscale must be a one-element float32 GPU tensor")
    if lay[1] == 1:
        cs = round_up(C, 8)
        rows = torch.empty((B,) + tuple(logits.shape[2:]) + (cs,), dtype=torch.float32, device=logits.device)
        grad = rows[..., :C].permute(0, rows.dim() - 1, *range(1, rows.dim() - 1))
        glay, gpad = (S * cs, 1, cs), cs
    else:
        grad = torch.empty_like(logits)
        glay, gpad = lay, 0
    a.q, a.gscale, a.grad = _ptr(q, "q"), _ptr(gscale, "gscale"), grad.data_ptr()
    a.g_b, a.g_c, a.g_v = glay
    a.g_pad = gpad
    a.c0, a.cc = 0, C
    _check(load().occd_lovasz_bwd(ctypes.byref(a), _stream()), "occd_lovasz_bwd")
    return grad


def lovasz_forward(logits, target, class_chunk=None, ignore=255):
    """Errors, sort and ranks for every class, `class_chunk` classes at a time over one cached scratch ->
    (q (N, C) float32, fg_count (C,) int64, loss_q (C,) int64).  No host read."""
    B, C = int(logits.shape[0]), int(logits.shape[1])
    N = lovasz_check_voxels(B * logits[0, 0].numel())
    cc = lovasz_chunk(C, class_chunk)
    sc = lovasz_scratch(N, cc, logits.device)
    q = torch.empty((N, C), dtype=torch.float32, device=logits.device)
    fg_count = torch.empty(C, dtype=torch.int64, device=logits.device)
    loss_q = torch.empty(C, dtype=torch.int64, device=logits.device)
    for c0 in range(0, C, cc):
        n = min(cc, C - c0)
        pairs = sc["pairs"][:, :, :n]
        lovasz_errors(logits, target, c0, n, pairs[0, 0], pairs[0, 1], ignore)
        keys, vals = sort_pairs(pairs[0, 0], pairs[0, 1], 0, LOVASZ_KEY_BITS, (pairs[1, 0], pairs[1, 1], sc["hist"]))
        lovasz_ranks(keys, vals, c0, q, fg_count, loss_q, sc["tsum"])
    return q, fg_count, loss_q


def lovasz_from_errors(err, fg, valid, raw=False):
    """Sort + ranks on ready-made errors: err (C, N) float32 in [0, 1], fg (C, N) uint8, valid (N,) uint8 ->
    (q (C, N) float32: (fg ? -g : g) of every valid voxel, 0 elsewhere; L_c (C,) float64 = loss_q / 2^60); with raw=True
    also (fg_count (C,) int64, loss_q (C,) int64: L_c in Q60).  The seam the exact tests go through: the keys are built
    here with torch, the kernels are those of the loss."""
    if err.dtype != torch.float32 or err.dim() != 2 or not err.is_cuda:
        raise RuntimeError("err must be a float32 (C, N) GPU tensor")
    C, N = (int(d) for d in err.shape)
    lovasz_check_voxels(N)
    if fg.dtype != torch.uint8 or tuple(fg.shape) != (C, N) or valid.dtype != torch.uint8 or tuple(valid.shape) != (N,):
        raise RuntimeError("fg must be uint8 (C, N) and valid uint8 (N,)")
    ok = valid.bool()[None].expand(C, N)
    bits = err.clamp(0.0, 1.0).contiguous().view(torch.int32)
    keys = torch.where(ok, LOVASZ_ONE_BITS - bits, torch.full_like(bits, LOVASZ_INVALID_KEY)).contiguous()
    idx = torch.arange(N, dtype=torch.int32, device=err.device)[None].expand(C, N)
    vals = torch.where(ok & fg.bool(), idx | torch.tensor(-(1 << 31), dtype=torch.int32, device=err.device), idx).contiguous()
    keys, vals = sort_pairs(keys, vals, 0, LOVASZ_KEY_BITS)
    q = torch.zeros((N, C), dtype=torch.float32, device=err.device)
    fg_count = torch.empty(C, dtype=torch.int64, device=err.device)
    loss_q = torch.empty(C, dtype=torch.int64, device=err.device)
    lovasz_ranks(keys, vals, 0, q, fg_count, loss_q)
    lc = loss_q.double() / float(1 << LOVASZ_Q)
    return (q.t(), lc, fg_count, loss_q) if raw else (q.t(), lc)


def cascade_tail(part, occ_off, wn, nbr):
    """ssc = part[..., :nbr] + conv3x3x3(softmax(part[..., occ_off:occ_off+2]), wn); returns a Vox with cs = ceil4(nbr)."""
    out = Vox.empty(part.batch, part.dims, nbr, part.buf.device, cs=round_up(nbr, 4))
    X, Y, Z = part.dims
    wc = wn.detach().float().contiguous()
    if _PROFILING:
        set_tag("%d @%dx%dx%d" % (nbr, X, Y, Z))
    _check(load().occd_cascade_tail_fwd(_f32(part.buf, "part"), _f32(wc, "wn"), _f32(out.buf, "out"), part.batch, X, Y,
                                        Z, part.cs, occ_off, out.cs, nbr, _stream()), "occd_cascade_tail_fwd")
    return out


class profile:
    """Context manager: HIP-event timing of every kernel launched inside (see occd_prof_*)."""

    def __init__(self):
        self.rows = {}

    def __enter__(self):
        global _PROFILING
        load().occd_prof_report(None, 0)  # drop stale records
        load().occd_prof_enable(1)
        _PROFILING = True
        return self

    def __exit__(self, *exc):
        global _PROFILING
        lib = load()
        lib.occd_prof_enable(0)
        _PROFILING = False
        set_tag(None)
        buf = (ProfRow * 512)()
        n = lib.occd_prof_report(buf, 512)
        if n < 0:
            raise RuntimeError("occd_prof_report failed")
        for i in range(min(n, 512)):
            r = buf[i]
            self.rows[r.tag.decode()] = dict(launches=r.launches, ms=r.ms, flops=r.flops, bytes=r.bytes)
        return False


def set_tag(tag):
    load().occd_prof_set_tag(tag.encode() if tag else None)
