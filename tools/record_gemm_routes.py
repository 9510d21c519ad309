"""Which entry point, operand forms and kernel every eval-path 2-D GEMM takes, for every switch setting, as a table
(tests/golden/gemm_routes.json).

    python tools/record_gemm_routes.py --device cpu  --out tests/golden/gemm_routes.json
    python tools/record_gemm_routes.py --device cuda --out tests/golden/gemm_routes.json     (adds its section)
    rocprofv3 --kernel-trace --output-format csv -d out -- python tools/record_gemm_routes.py --launch out/launches.json
    python tools/record_gemm_routes.py --kernels out/launches.json <kernel_trace.csv> --out tests/golden/gemm_routes.json

Host table: the real call sites (efficientnet.expand_gemm / project_conv, UpSampleBN._first_conv_upconv / _conv_bn_act,
DecoderBN._conv2_merged, bare hip.matmul) are driven over CASES crossed with settings(); hip.gemm_x3, hip.gemm_x3_splitk,
hip.conv1x1, torch.matmul, GemmPacked.__init__ and pw_pack_weights are replaced by recorders (stubbed()), so nothing is
launched: a run touches the device for allocations, the folding of the weights and the finite-weights test of the f16x2
image.  Per case and setting the table holds the launch lines (entry point, form of A, form of B, epilogue operands,
M x N x K and batch, the K21 plan) and the pack lines (kind).  Caches are dropped between settings: a setting is recorded as
a fresh process would see it.

Kernel table: every distinct (M, N, K, batch, pre, plain epilogue) that reaches occd_gemm_f32x3 with tile_hint 0 under the
default setting and under GEMM_X3_PANEL=0 is launched once for real (--launch, under rocprofv3 --kernel-trace with nothing
else enabled), and --kernels joins the trace to the launches: kernel name, grid, workgroup size and LDS bytes.  It is the
record of what the library's own hint-0 rule picks; tests/test_gemm_routes.py holds occd_gemm_f32x3_route against it.

The committed table was recorded before the dispatch was touched (the commit is named in the table's "recorded_at").
"""
import argparse
import contextlib
import csv
import json
import os
import re
import sys
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from occdepth_amd import fused, hip  # noqa: E402
from occdepth_amd.models import efficientnet as en  # noqa: E402
from occdepth_amd.models import unet2d  # noqa: E402

UP = unet2d.UpSampleBN
FOLD = 1 << 40            # UPCONV_FOLD_BELOW large enough to take the folded 2-D tap GEMM on every case

# (label, switches that differ from the defaults): each single switch, and both where two of them meet in one predicate
_SETTINGS = (
    ("default", {}),
    ("split=bf16x3", dict(GEMM_SPLIT="bf16x3")),
    ("x3=0", dict(GEMM_X3=False)),
    ("panel=0", dict(GEMM_X3_PANEL=False)),
    ("pack=1", dict(GEMM_X3_PACK=True)),
    ("tile_f16x2=0", dict(TILE_F16X2=False)),
    ("splitk=0", dict(PW_PROJECT_SPLITK=False)),
    ("k16=0", dict(PW_PROJECT_K16=False)),
    ("wino_cm=0", dict(WINO_CM=False)),
    ("fold", dict(UPCONV_FOLD_BELOW=FOLD)),
    ("split=bf16x3 panel=0", dict(GEMM_SPLIT="bf16x3", GEMM_X3_PANEL=False)),
    ("split=bf16x3 pack=1", dict(GEMM_SPLIT="bf16x3", GEMM_X3_PACK=True)),
    ("split=bf16x3 splitk=0", dict(GEMM_SPLIT="bf16x3", PW_PROJECT_SPLITK=False)),
    ("split=bf16x3 fold", dict(GEMM_SPLIT="bf16x3", UPCONV_FOLD_BELOW=FOLD)),
    ("panel=0 pack=1", dict(GEMM_X3_PANEL=False, GEMM_X3_PACK=True)),
    ("panel=0 tile_f16x2=0", dict(GEMM_X3_PANEL=False, TILE_F16X2=False)),
    ("panel=0 fold", dict(GEMM_X3_PANEL=False, UPCONV_FOLD_BELOW=FOLD)),
    ("splitk=0 k16=0", dict(PW_PROJECT_SPLITK=False, PW_PROJECT_K16=False)),
    ("x3=0 fold", dict(GEMM_X3=False, UPCONV_FOLD_BELOW=FOLD)),
)
DEFAULTS = dict(GEMM_SPLIT="f16x2", GEMM_X3=True, GEMM_X3_PANEL=True, GEMM_X3_PACK=False, TILE_F16X2=True, WINO_CM=True,
                PW_PROJECT_SPLITK=True, PW_PROJECT_K16=True, UPCONV_FOLD_BELOW=0)
# where each switch lives: (object, attribute); GEMM_SPLIT goes through its setter
_HOME = {"GEMM_X3": hip, "GEMM_X3_PANEL": hip, "GEMM_X3_PACK": hip, "TILE_F16X2": hip, "WINO_CM": hip,
         "PW_PROJECT_SPLITK": en, "PW_PROJECT_K16": en, "UPCONV_FOLD_BELOW": UP}


def settings():
    """[(label, dict of all switches)]."""
    return [(label, dict(DEFAULTS, **s)) for label, s in _SETTINGS]


def _current():
    s = {n: getattr(home, n) for n, home in _HOME.items()}
    s["GEMM_SPLIT"] = fused.GEMM_SPLIT
    return s


def apply_switches(s):
    for n, v in s.items():
        if n == "GEMM_SPLIT":
            fused.set_gemm_split(v)
        else:
            setattr(_HOME[n], n, v)


@contextlib.contextmanager
def switches(s):
    saved = _current()
    try:
        apply_switches(s)
        yield
    finally:
        apply_switches(saved)


def _form(t):
    if isinstance(t, hip.GemmPacked):
        return t.split
    return {torch.float32: "f32"}.get(t.dtype, str(t.dtype))


def _dims(a, b):
    pa, pb = isinstance(a, hip.GemmPacked), isinstance(b, hip.GemmPacked)
    nb_a = a.batch if pa else (a.shape[0] if a.dim() == 3 else None)
    nb_b = b.batch if pb else (b.shape[0] if b.dim() == 3 else None)
    M, K = (a.rows, a.K) if pa else (a.shape[-2], a.shape[-1])
    N = b.rows if pb else b.shape[-1]
    return int(M), int(N), int(K), nb_a, nb_b


def _blank(shape, like):
    """A result of `shape` that owns one element (nothing reads it on the GPU paths; the CPU fallbacks run on small shapes)."""
    return torch.empty(1, device=like.device, dtype=torch.float32).expand(tuple(shape))


def _epilogue(bias=None, act=None, res=None, k_scale=None, bias_n=None, out=None):
    parts = [n for n, v in (("bias", bias), ("res", res), ("kscale", k_scale), ("bias_n", bias_n)) if v is not None]
    if act is not None:
        parts.append("act=" + act)
    if out is not None:
        parts.append("out=" + ("dense" if out.is_contiguous() else "strided"))
    return " ".join(parts) if parts else "-"


_SILENT = ("wino_input_transform", "wino_input_transform_cm", "wino_output_transform", "wino_output_transform_cm",
           "upconv_gather", "conv2d_3x3_fused", "affine_act")


@contextlib.contextmanager
def stubbed(log, packs=None, launch=None):
    """The GEMM entry points and the weight packers replaced: launches append one line to `log`, packs (kind) to `packs`.
    launch: a list -> the real GemmPacked and the real hip.gemm_x3 run for every hint-0 launch of a geometry not seen before,
    and `launch` receives its (M, N, K, batch, pre, plain) record (the kernel table's --launch mode)."""
    real = dict(gemm_x3=hip.gemm_x3, gemm_x3_splitk=hip.gemm_x3_splitk, conv1x1=hip.conv1x1, pw_pack_weights=hip.pw_pack_weights,
                init=hip.GemmPacked.__init__, matmul=torch.matmul, conv2d=torch.nn.functional.conv2d, wino_pack=fused.wino_pack)
    real.update({n: getattr(hip, n) for n in _SILENT})
    note = packs.append if packs is not None else (lambda kind: None)

    def packed_init(self, w, role, split="bf16x3"):
        if split == "f16x2" and not bool(torch.isfinite(w).all()):
            raise ValueError("occd_gemm_f16x2_pack: a weight is not finite")      # (the pack's own test, on the real weights)
        if launch is not None:
            real["init"](self, w, role, split)
        else:
            self.role, self.batch, self.split = role, (w.shape[0] if w.dim() == 3 else None), split
            self.rows, self.K = (w.shape[-2], w.shape[-1]) if role == "a" else (w.shape[-1], w.shape[-2])
            self.shape, self.per, self.buf = tuple(w.shape), 0, torch.empty(0, device=w.device)
        note("%s-%s %dx%d%s" % (split, role, self.rows, self.K, " b%d" % self.batch if self.batch else ""))

    def pw_pack(w, scale=None):
        note("k11 %dx%d" % (w.shape[0], w.shape[1]))
        return torch.empty(0, device=w.device)

    def gemm_x3(a, b, bias=None, act=None, slope=0.01, out=None, tile_hint=0, plain_bf16=False, res=None, k_scale=None,
                sigmoid_a=False, bias_n=None):
        M, N, K, nb_a, nb_b = _dims(a, b)
        batch = nb_a or nb_b or 1
        log.append("gemm_x3 A=%s B=%s %s %dx%dx%d b%d%s" % (_form(a), _form(b), _epilogue(bias, act, res, k_scale, bias_n, out),
                                                          M, N, K, batch, " hint%d" % tile_hint if tile_hint else ""))
        if launch is not None and tile_hint == 0:
            pa, pb = isinstance(a, hip.GemmPacked), isinstance(b, hip.GemmPacked)
            pre = (hip.GEMM_PRE_F16X2 if a.split == "f16x2" else 1) if pa else 2 if pb else 0
            plain = int(res is None and k_scale is None and bias_n is None and not sigmoid_a)
            key = dict(M=M, N=N, K=K, batch=batch, pre=pre, plain=plain)
            if key not in launch:
                launch.append(key)
                return real["gemm_x3"](a, b, bias=bias, act=act, slope=slope, out=out, res=res, k_scale=k_scale, bias_n=bias_n)
        if out is not None:
            return out
        y = _blank((batch, M, N), b.buf if isinstance(b, hip.GemmPacked) else b)
        return y[0] if nb_a is None and nb_b is None else y

    def gemm_x3_splitk(a, b, bias=None, act=None, slope=0.01, out=None, res=None, k_scale=None, plan=None):
        batch = b.shape[0] if b.dim() == 3 else 1
        M, K, N = a.rows, a.K, b.shape[-1]
        if plan is None:
            plan = hip.gemm_x3_splitk_plan(M, N, K, batch)[:3]
        log.append("gemm_x3_splitk A=%s B=%s %s %dx%dx%d b%d plan=%d,%d,%d" % ((_form(a), _form(b), _epilogue(bias, act, res, k_scale, None, out),
                                                                             M, N, K, batch) + tuple(plan)))
        y = _blank((batch, M, N), b)
        return y[0] if b.dim() == 2 else y

    def conv1x1(x, wpk, cout, shift=None, act=None, slope=0.01, gate=None, res=None, tile_hint=0, out=None, nhwc=False):
        ep = [n for n, v in (("shift", shift), ("gate", gate), ("res", res)) if v is not None] + (["act=" + act] if act else [])
        log.append("conv1x1 k11 %s %d<-%d @%dx%dx%d" % (" ".join(ep) or "-", cout, x.shape[1], x.shape[0], x.shape[2], x.shape[3]))
        return _blank((x.shape[0], cout) + tuple(x.shape[2:]), x)

    def matmul(a, b):
        M, N, K, nb_a, nb_b = _dims(a, b)
        log.append("torch.matmul A=%s B=%s %dx%dx%d b%d" % (_form(a), _form(b), M, N, K, nb_a or nb_b or 1))
        return _blank(torch.broadcast_shapes(a.shape[:-2], b.shape[:-2]) + (M, N), a)

    def conv2d(x, w, bias=None, stride=1, padding=0, *args, **kw):
        log.append("F.conv2d %d<-%d k%d @%dx%dx%d" % (w.shape[0], w.shape[1], w.shape[2], x.shape[0], x.shape[2], x.shape[3]))
        p = padding if isinstance(padding, int) else padding[0]
        k = w.shape[2]
        return _blank((x.shape[0], w.shape[0], x.shape[2] + 2 * p - k + 1, x.shape[3] + 2 * p - k + 1), x)

    def silent(name):
        def run(x, *a, **kw):
            if name == "wino_input_transform":
                B, C, H, W = x.shape
                ths = a[1] if len(a) > 1 and a[1] is not None else (H + 1) // 2 - (a[0] if a else 0)
                return torch.empty((16, B * ths * ((W + 1) // 2), C), device=x.device)
            if name == "wino_input_transform_cm":
                B, C, H, W = x.shape
                T = B * ((H + 1) // 2) * ((W + 1) // 2)
                return torch.empty((16, C, hip.round_up(T, 32)), device=x.device)[..., :T]
            if name in ("wino_output_transform", "wino_output_transform_cm"):
                return kw["out"] if kw.get("out") is not None else _blank(a[0], x)
            if name == "upconv_gather":
                return _blank((x.shape[1 if kw.get("batch_inner") else 0], a[0]) + tuple(a[1]), x)      # z, cout, size
            if name == "conv2d_3x3_fused":
                return _blank((x.shape[0], a[1]) + tuple(x.shape[2:]), x)
            return x                                                       # affine_act: shape-preserving
        return run

    try:
        hip.gemm_x3, hip.gemm_x3_splitk, hip.conv1x1, hip.pw_pack_weights = gemm_x3, gemm_x3_splitk, conv1x1, pw_pack
        hip.GemmPacked.__init__ = packed_init
        torch.matmul, torch.nn.functional.conv2d = matmul, conv2d
        fused.wino_pack = lambda w, scale=None: None
        for n in _SILENT:
            setattr(hip, n, silent(n))
        yield
    finally:
        hip.gemm_x3, hip.gemm_x3_splitk, hip.conv1x1, hip.pw_pack_weights = (real["gemm_x3"], real["gemm_x3_splitk"], real["conv1x1"],
                                                                            real["pw_pack_weights"])
        hip.GemmPacked.__init__ = real["init"]
        torch.matmul, torch.nn.functional.conv2d = real["matmul"], real["conv2d"]
        fused.wino_pack = real["wino_pack"]
        for n in _SILENT:
            setattr(hip, n, real[n])


def _c(kind, M, N, K, batch=2, **kw):
    """A case: `kind` of call site; M rows x N columns (pixels of ONE image) x K; hw = (h, w) with h * w = N where the site needs
    a map (default: the squarest h x w = N); flags: inf (one Inf weight), nc (the non-contiguous operand), res (with skip), kscale,
    pad (expand: result rows on the 128-byte pitch), strips (wino: the strip mode)."""
    return dict(kind=kind, M=M, N=N, K=K, batch=batch, **kw)


def _hw(n):
    """(h, w), h * w = n, as square as the divisors allow (a map of n pixels)."""
    h = int(n ** 0.5)
    while n % h:
        h -= 1
    return h, n // h


CASES = {}
# the config-2 frame at batch 2 -- tap GEMMs (rows 9 Cout), expands, projects, the channel-major Winograd products, the head
for _m, _n, _k in ((720, 112850, 160), (1440, 28365, 320), (2880, 7191, 640), (5760, 1848, 1280), (11520, 574, 2560)):
    CASES[f"tap_{_m}x{_n}x{_k}"] = _c("tap", _m, _n, _k)
for _m, _n, _k in ((192, 112850, 32), (288, 28365, 48), (480, 7191, 80), (1344, 1848, 224), (2304, 468, 384), (3840, 468, 640)):
    CASES[f"expand_{_m}x{_n}x{_k}"] = _c("expand", _m, _n, _k, pad=True)
for _m, _n, _k in ((48, 28365, 288), (80, 7191, 480), (160, 1848, 960), (224, 1848, 1344), (384, 468, 1344), (384, 468, 2304),
                   (640, 468, 3840), (32, 112850, 32)):
    CASES[f"project_{_m}x{_n}x{_k}"] = _c("project", _m, _n, _k)
    CASES[f"project_{_m}x{_n}x{_k}_res"] = _c("project", _m, _n, _k, res=True)
CASES.update({
    "wino_1280_1280_24x77": _c("wino", 1280, 24 * 77, 1280, hw=(24, 77)),
    "wino_640_640_47x153": _c("wino", 640, 47 * 153, 640, hw=(47, 153)),
    "wino_256_256_12x39": _c("wino", 256, 12 * 39, 256, hw=(12, 39)),                  # wino_cm_wins turns it down
    "wino_512_512_24x77": _c("wino", 512, 24 * 77, 512, hw=(24, 77)),                  # cin at the rule's edge, too few workgroups
    "wino_1280_1280_strips": _c("wino", 1280, 24 * 77, 1280, hw=(24, 77), strips=True),
    "wino_1280_1280_inf_weight": _c("wino", 1280, 24 * 77, 1280, hw=(24, 77), inf=True),
    "head_2560x574x640": _c("head", 2560, 14 * 41, 640, hw=(12, 39)),                   # (12, 39) + conv2's padding = 14 x 41 = 574
    "head_inf_weight": _c("head", 2560, 14 * 41, 640, hw=(12, 39), inf=True),
    "head_c_not_8": _c("head", 64, 5 * 6, 20, hw=(3, 4)),
    # both sides of every threshold.  PANEL_MIN_ROWS:
    "expand_255_rows": _c("expand", 255, 4100, 64, pad=True), "expand_256_rows": _c("expand", 256, 4100, 64, pad=True),
    "matmul_255x4100x352": _c("matmul", 255, 4100, 352, batch=1),
    # the library's panel rule: K <= 352, K <= 848 with ceil(N / 64) * batch * ceil(ceil(M / 32) / 8) <= 512
    "matmul_256x4100x352": _c("matmul", 256, 4100, 352, batch=1), "matmul_256x4100x360": _c("matmul", 256, 4100, 360, batch=1),
    "matmul_256x4100x848": _c("matmul", 256, 4100, 848, batch=1), "matmul_256x4100x856": _c("matmul", 256, 4100, 856, batch=1),
    "matmul_small_launch_512": _c("matmul", 256, 64 * 256, 848), "matmul_small_launch_514": _c("matmul", 256, 64 * 256 + 1, 848),
    # _presplit_launch: K >= 512 and ceil(M / 256) * ceil(N / 128) * batch >= 320
    "matmul_presplit_k504": _c("matmul", 2880, 7191, 504), "matmul_presplit_k512": _c("matmul", 2880, 7191, 512),
    "matmul_presplit_320wg": _c("matmul", 2560, 128 * 16, 1024), "matmul_presplit_319wg": _c("matmul", 2816, 128 * 29, 1024, batch=1),
    "matmul_2560x468x640": _c("matmul", 2560, 468, 640),
    "matmul_res": _c("matmul", 2304, 468, 384, res=True), "matmul_kscale": _c("matmul", 2304, 468, 384, kscale=True),
    "matmul_small_res_kscale": _c("matmul", 48, 1500, 64, res=True, kscale=True),
    "matmul_role_b": _c("matmul_b", 936, 1280, 1280, batch=16),
    "matmul_inf_weight": _c("matmul", 2304, 468, 384, inf=True),
    "matmul_a_unaligned": _c("matmul", 2304, 468, 384, nc="a"),
    # tile_f16x2_wins: >= 48 rows on >= 3000 columns over the batch
    "expand_47_rows": _c("expand", 47, 4000, 64, pad=True), "expand_48_rows": _c("expand", 48, 4000, 64, pad=True),
    "expand_2999_cols": _c("expand", 192, 2999, 32, batch=1, pad=True), "expand_3000_cols": _c("expand", 192, 3000, 32, batch=1, pad=True),
    # the K16 project: >= 3000 pixels over the batch, >= 48 output channels
    "project_47_rows": _c("project", 47, 4000, 288), "project_48_rows": _c("project", 48, 4000, 288),
    "project_2999_cols": _c("project", 48, 2999, 288, batch=1, res=True), "project_3000_cols": _c("project", 48, 3000, 288, batch=1, res=True),
    "project_1499_cols_b2": _c("project", 48, 1499, 288, res=True), "project_1500_cols_b2": _c("project", 48, 1500, 288, res=True),
    # splitk_f16x2_wins: 5 row tiles x 27 / 28 steps per chunk under the library's plan (135 / 140 tile-steps; 139 has no plan)
    "project_135_tile_steps": _c("project", 160, 1848, 864, res=True), "project_140_tile_steps": _c("project", 160, 1848, 896, res=True),
    # K21: C >= 768 on at most 8000 pixels over the batch
    "project_k760": _c("project", 160, 1848, 760, res=True), "project_k768": _c("project", 160, 1848, 768, res=True),
    "project_8000_pixels": _c("project", 160, 4000, 960, res=True), "project_8008_pixels": _c("project", 160, 4004, 960, res=True),
    "project_c_not_8": _c("project", 48, 28365, 292), "expand_c_not_8": _c("expand", 288, 28365, 44, pad=True),
    "project_hw_3": _c("project", 384, 3, 2304, res=True), "expand_hw_3": _c("expand", 2304, 3, 384, pad=True),
    "project_y_strided": _c("project", 160, 1848, 960, res=True, nc="y"), "project_gate_strided": _c("project", 160, 1848, 960, res=True, nc="gate"),
    "project_res_strided": _c("project", 160, 1848, 960, res=True, nc="res"),
    "project_k16_y_strided": _c("project", 48, 28365, 288, res=True, nc="y"), "project_k16_res_strided": _c("project", 48, 28365, 288, res=True, nc="res"),
    "project_k16_gate_strided": _c("project", 48, 28365, 288, res=True, nc="gate"),
    "expand_x_strided": _c("expand", 288, 28365, 48, pad=True, nc="x"),
    "expand_dense_out": _c("expand", 288, 28365, 48, pad=False),
    "project_inf_weight": _c("project", 160, 1848, 960, res=True, inf=True), "project_k16_inf_weight": _c("project", 48, 28365, 288, res=True, inf=True),
    "expand_inf_weight": _c("expand", 2304, 468, 384, pad=True, inf=True), "expand_small_inf_weight": _c("expand", 192, 112850, 32, pad=True, inf=True),
    "tap_inf_weight": _c("tap", 1440, 28365, 320, inf=True),
    "tap_batch1": _c("tap", 2880, 7191, 640, batch=1),
})
# the CPU section holds the fallbacks: no size decides anything there, so it runs on maps of at most CPU_MAX_PIXELS pixels and
# matrices of at most CPU_MAX_ROWS x CPU_MAX_K (K keeps its remainder mod 8, a tap matrix its nine taps)
CPU_MAX_PIXELS, CPU_MAX_ROWS, CPU_MAX_K = 600, 72, 64


def _cpu_case(c):
    c = dict(c)
    c["M"] = min(c["M"], CPU_MAX_ROWS)
    c["K"] = c["K"] if c["K"] <= CPU_MAX_K else CPU_MAX_K + c["K"] % 8
    if c["kind"] == "matmul_b":
        c["N"] = min(c["N"], CPU_MAX_ROWS)
    return c


def _map(c, device):
    hw = c.get("hw") or _hw(c["N"])
    if device == "cpu" and hw[0] * hw[1] > CPU_MAX_PIXELS:
        hw = (12, 39)
    return hw


def _conv(cin, cout, k, device, inf, **kw):
    conv = nn.Conv2d(cin, cout, k, **kw).to(device)
    if inf:
        with torch.no_grad():
            conv.weight[1, 2, 0, 0] = float("inf")
    return conv


def _strided(t):
    """The same values behind a non-contiguous view (every second column of a buffer twice as wide)."""
    return torch.empty(t.shape[:-1] + (2 * t.shape[-1],), device=t.device)[..., ::2]


def build_case(c, device):
    """The modules and inputs of a case (built once, shared by all its settings) -> a function that drops the operand caches
    and calls the site."""
    torch.manual_seed(0)
    c = _cpu_case(c) if device == "cpu" else c
    M, K, B, kind, nc, inf = c["M"], c["K"], c["batch"], c["kind"], c.get("nc"), c.get("inf", False)
    with torch.no_grad():
        if kind in ("matmul", "matmul_b"):
            N = c["N"] if device != "cpu" else min(c["N"], CPU_MAX_PIXELS)
            if kind == "matmul_b":                      # the Winograd-domain product of the present form: V (16, T, Cin) @ U (16, Cin, Cout)
                v, u = torch.empty(B, M, K, device=device), torch.randn(B, K, c["N"], device=device)
                return lambda: hip.matmul(v, hip.GemmWeights(u, "b"))
            w = torch.randn(M, K + (4 if nc == "a" else 0), device=device)
            if inf:
                w[1, 2] = float("inf")
            w = w[:, :K] if nc == "a" else w
            b = torch.empty((B, K, N) if B > 1 else (K, N), device=device)
            shape = (B, M, N) if B > 1 else (M, N)                     # (N: the clipped one on the CPU)
            res = torch.empty(shape, device=device) if c.get("res") else None
            ks = torch.empty(B, K, device=device) if c.get("kscale") else None

            def run():
                hip.matmul(hip.GemmWeights(w, "a", split="switch"), b, res=res, k_scale=ks)
                hip.matmul(hip.GemmWeights(w, "a"), b, res=res, k_scale=ks)           # (split None: the three-term image)
            return run
        h, wd = _map(c, device)
        if kind in ("expand", "project"):
            conv, bn = _conv(K, M, 1, device, inf, bias=False), nn.BatchNorm2d(M).to(device).eval()
            x = torch.empty(B, K, h, wd, device=device)
            x = _strided(x) if nc in ("x", "y") else x
            owner = types.SimpleNamespace()
            if kind == "expand":
                def run():
                    owner.__dict__.clear()
                    en.expand_gemm(owner, conv, bn, x, "swish", pad_out=c.get("pad", False))
                return run
            gate = torch.empty(B, K, device=device)
            gate = _strided(gate) if nc == "gate" else gate
            res = torch.empty(B, M, h, wd, device=device) if c.get("res") else None
            res = _strided(res) if nc == "res" else res

            def run():
                owner.__dict__.clear()
                en.project_conv(owner, conv, bn, x, gate, res)
            return run
        if kind == "tap":
            cout, skipc = M // 9, 8
            up = UP(skip_input=K + skipc, output_features=cout).to(device).eval()
            if inf:
                up._net[0].weight[1, 2, 0, 0] = float("inf")
            x, skip = torch.empty(B, K, h, wd, device=device), torch.empty(B, skipc, 2 * h, 2 * wd, device=device)

            def run():
                for k in [k for k in up.__dict__ if k.endswith("_cache")]:
                    del up.__dict__[k]
                up._first_conv_upconv(x, skip, up._net[0], up._net[1], up._net[2])
            return run
        if kind == "wino":
            up = types.SimpleNamespace(FUSED=UP.FUSED, FUSED_MIN_PIXELS=UP.FUSED_MIN_PIXELS, WINOGRAD=True, WINOGRAD_MIN_CIN=UP.WINOGRAD_MIN_CIN,
                                       WINOGRAD_MAX_PIXELS=0 if c.get("strips") else UP.WINOGRAD_MAX_PIXELS,
                                       WINOGRAD_HIRES_MIN_CIN=64, WINOGRAD_HIRES_PIXELS=1 << 40, WINOGRAD_STRIP_MB=64.0)
            up._wino_operands = types.MethodType(UP._wino_operands, up)
            conv, bn, act = _conv(K, M, 3, device, inf, padding=1), nn.BatchNorm2d(M).to(device).eval(), nn.LeakyReLU()
            f = torch.empty(B, K, h, wd, device=device)

            def run():
                up.__dict__.pop("_wino_cache", None)
                UP._conv_bn_act(up, f, conv, bn, act)
            return run
        if kind == "head":
            dec = types.SimpleNamespace(conv2=nn.Conv2d(M, M, 1, padding=1).to(device))
            head = _conv(K, M, 1, device, inf, bias=False)
            f = torch.empty(B, K, h, wd, device=device)

            def run():
                dec.__dict__.pop("_merged_head", None)
                unet2d.DecoderBN._conv2_merged(dec, f, head)
            return run
    raise ValueError(kind)


def record(device, names=None, launch=None, only=None):
    """{case: [(launch lines, pack lines) per setting, in settings() order]} on `device`."""
    table = {}
    for name, c in CASES.items():
        if names is not None and name not in names:
            continue
        run = build_case(c, device)
        rows = []
        for label, s in settings():
            if only is not None and label not in only:
                continue
            log, packs = [], []
            with switches(s), stubbed(log, packs, launch), torch.no_grad():
                run()
            rows.append([log, packs])
        table[name] = rows
    return table


KERNEL_SETTINGS = ("default", "panel=0")


def read_trace(path):
    """[(kernel name, grid in workgroups (x, y), workgroup size, LDS bytes)] of the K16 launches of a kernel-trace CSV, in order."""
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = []
    for r in rows:
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        if not re.search(r"gemm_x3_(panel_|ws_)?kernel<", name):
            continue
        wg = int(r.get("Workgroup_Size_X") or r["Workgroup_Size"])
        gx = int(r.get("Grid_Size_X") or r["Grid_Size"])
        gy = int(r.get("Grid_Size_Y") or 1)
        if "Grid_Size_X" not in r:                   # one total: threads over all dimensions
            gx, gy = gx // wg, 0
        else:
            gx //= wg
        out.append(dict(kernel=re.sub(r"^void |\(.*$", "", name), grid=[gx, gy], wg=wg, lds=int(r["LDS_Block_Size"])))
    return out


def _store(doc, device, table):
    # the sequences repeat: store each distinct one once and the table as indices into that list
    seqs = doc.setdefault("sequences", [])
    index = {json.dumps(s): i for i, s in enumerate(seqs)}

    def ref(seq):
        key = json.dumps(seq)
        if key not in index:
            index[key] = len(seqs)
            seqs.append(seq)
        return index[key]
    doc[device] = {name: [[ref(log), ref(packs)] for log, packs in rows] for name, rows in table.items()}
    doc["settings"] = [label for label, _ in settings()]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", choices=("cpu", "cuda"))
    ap.add_argument("--launch", help="launch the kernel table's geometries for real; write their list here")
    ap.add_argument("--kernels", nargs=2, metavar=("LAUNCHES", "TRACE"), help="join the --launch list with the kernel-trace CSV")
    ap.add_argument("--recorded-at", help="the commit the table is recorded at")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.launch:
        launch = []
        record("cuda", launch=launch, only=KERNEL_SETTINGS)
        torch.cuda.synchronize()
        with open(a.launch, "w") as f:
            json.dump(launch, f)
        print(f"{len(launch)} geometries launched -> {a.launch}")
        return
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.kernels:
        with open(a.kernels[0]) as f:
            launches = json.load(f)
        trace = read_trace(a.kernels[1])
        assert len(trace) == len(launches), (len(trace), len(launches))
        doc["kernels"] = [dict(l, **t) for l, t in zip(launches, trace)]
        print(f"{len(launches)} kernel rows")
    else:
        table = record(a.device)
        _store(doc, a.device, table)
        print(f"{a.device}: {len(table)} cases x {len(settings())} settings, {len(doc['sequences'])} distinct sequences -> {a.out}")
    if a.recorded_at:
        doc["recorded_at"] = a.recorded_at
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
