"""CPU: libocc_hip.so builds, loads, and exports exactly what include/occdepth_amd.h declares; the
ctypes structures occdepth_amd/abi.py derives from the header have the C layout (checked against gcc's
sizeof/offsetof); the parser accepts the header's subset of C and raises on everything else."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "occdepth_amd.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(occd_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(hip_lib):
    from occdepth_amd import hip
    names = declared_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in the header but not exported"
        assert n in hip.EXPORTS, f"{n} has no ctypes prototype"
    assert sorted(hip.EXPORTS) == names
    assert hip_lib.occd_abi_version() == hip.ABI_VERSION
    assert hip_lib.occd_strerror(-1).decode().startswith("invalid")


def test_argument_validation_without_gpu(hip_lib):
    """Pure host-side argument checks (no launch happens for invalid arguments)."""
    from occdepth_amd import hip
    assert hip_lib.occd_conv3d_fwd(None, None) == -1
    a = hip.Conv3dArgs()
    assert hip_lib.occd_conv3d_fwd(ctypes.byref(a), None) == -1
    assert hip_lib.occd_lift_fwd(None, None) == -1
    assert hip_lib.occd_flosp_sample_fwd(None, None) == -1
    assert hip_lib.occd_packed_weight_floats(32, 32, 27) == 27 * 4 * 1 * 256
    assert hip_lib.occd_packed_weight_floats(20, 34, 27) == 27 * 5 * 1 * 256
    assert hip_lib.occd_packed_weight_floats(0, 1, 1) < 0


def test_ctypes_structs_match_c_layout(tmp_path):
    from occdepth_amd import abi
    structs = abi.STRUCTS                   # every structure the header declares
    assert sorted(structs) == sorted(re.findall(r"^typedef struct (\w+)", open(HEADER).read(), flags=re.M)) and len(structs) >= 21
    rename = {"inp": "in"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {rename.get(fname, fname)}));')
    lines += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", str(src), "-o", str(exe)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    for cname, st in structs.items():
        assert int(out[cname]) == ctypes.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(st, fname).offset, f"{cname}.{fname}"


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from occdepth_amd import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="missing"):
        hip.load()


def test_new_entry_points_validate_arguments(hip_lib):
    """Host-side validation of the 2-D helper / projection / tail entry points (no launch for bad arguments)."""
    import ctypes
    assert hip_lib.occd_affine_act_nchw(None, None, None, None, None, 1, 1, 1, 0, 0.0, 0, None) == -1
    assert hip_lib.occd_dwconv2d_nchw(None, None, None, None, None, 1, 1, 1, 1, 3, 1, 0, 0, 1, 1, 0, None) == -1
    assert hip_lib.occd_upsample_bilinear_cat_nchw(None, None, None, 1, 1, 0, 1, 1, 1, 1, None) == -1
    assert hip_lib.occd_cascade_tail_fwd(None, None, None, 1, 1, 1, 1, 24, 20, 20, 20, None) == -1
    assert hip_lib.occd_argmax_channels(None, 1, 4, 0, 4, None, None, None) == -1
    e = (ctypes.c_double * 16)()
    assert hip_lib.occd_project_voxels(ctypes.addressof(e), None, None, 0.2, 1, 1, 1, 1, 1, None, None, None, None) == -1


def test_training_entry_points_validate_arguments(hip_lib):
    """Loss statistics / confusion / weight-gradient entry points reject bad arguments before any launch."""
    import ctypes
    from occdepth_amd import hip
    assert hip_lib.occd_ssc_stats_len(20, 64) == 3 * 20 + 3 + 64 * 20
    assert hip_lib.occd_ssc_loss_stats_fwd(None, None, None, None, None, 1, 20, 8, 0, 0, None) == -1
    one = ctypes.c_float(0.0)
    ptr = ctypes.addressof(one)
    assert hip_lib.occd_ssc_loss_stats_fwd(ptr, ptr, None, None, ptr, 1, 33, 8, 0, 0, None) == -1      # C > 32
    assert hip_lib.occd_ssc_loss_stats_fwd(ptr, ptr, None, None, ptr, 1, 20, 8, 4, 0, None) == -1       # masks missing
    assert hip_lib.occd_ssc_loss_stats_bwd(ptr, ptr, None, None, None, ptr, 1, 20, 8, 0, 0, None) == -1
    assert hip_lib.occd_ssc_confusion(ptr, ptr, ptr, ptr, 1, 20, 8, None) == -1                         # both predictions
    assert hip_lib.occd_ssc_confusion(None, None, ptr, ptr, 1, 20, 8, None) == -1                       # neither
    a = hip.WgradArgs()
    assert hip_lib.occd_conv3d_wgrad_workspace_floats(ctypes.byref(a)) == -1
    a.x = a.gy = ptr
    a.batch, a.X, a.Y, a.Z, a.cin, a.x_cs = 1, 4, 4, 8, 32, 32
    a.Xo, a.Yo, a.Zo, a.cout, a.gy_cs = 4, 4, 8, 32, 32
    a.kx = a.ky = a.kz = 3
    a.sx = a.sy = a.sz = a.dx = a.dy = a.dz = 1
    a.px = a.py = a.pz = 1
    need = hip_lib.occd_conv3d_wgrad_workspace_floats(ctypes.byref(a))
    assert need > 0 and need % (27 * 1024) == 0
    assert hip_lib.occd_conv3d_wgrad(ctypes.byref(a), None) == -1                                        # no dw / workspace
    a.kx = 6
    a.ky = 6
    assert hip_lib.occd_conv3d_wgrad_workspace_floats(ctypes.byref(a)) == -1                             # > 32 taps


def test_winograd_entry_points_validate_arguments(hip_lib):
    assert hip_lib.occd_wino_input_transform_nchw(None, None, 1, 8, 4, 4, 0, 2, None) == -1
    assert hip_lib.occd_wino_output_transform_nchw(None, None, None, None, None, 1, 8, 4, 4, 0, 2, 0, 0.0, 0, None) == -1
    import ctypes
    one = ctypes.c_float(0.0)
    ptr = ctypes.addressof(one)
    assert hip_lib.occd_wino_input_transform_nchw(ptr, ptr, 0, 8, 4, 4, 0, 2, None) == -1
    assert hip_lib.occd_wino_input_transform_nchw(ptr, ptr, 1, 8, 4, 4, 1, 2, None) == -1                            # strip past the image
    assert hip_lib.occd_wino_output_transform_nchw(ptr, None, None, None, ptr, 1, 8, 4, 4, 0, 2, 7, 0.0, 0, None) == -1     # act code


def test_round2_2d_entry_points_validate_arguments(hip_lib):
    """K10 / K11 / SE-gate / pooled depthwise entry points: argument checks happen before any launch."""
    import ctypes
    from occdepth_amd import hip
    assert hip_lib.occd_wino_packed_floats(80, 163) == 21 * 16 * 3 * 256
    assert hip_lib.occd_wino_packed_floats(0, 8) < 0
    assert hip_lib.occd_wino_conv3x3_fwd(None, None) == -1
    w = hip.WinoArgs()
    assert hip_lib.occd_wino_conv3x3_fwd(ctypes.byref(w), None) == -1
    one = ctypes.c_float(0.0)
    ptr = ctypes.addressof(one)
    w.x = w.upk = w.y = ptr
    w.batch, w.cin, w.cout, w.H, w.W, w.act = 1, 8, 8, 4, 4, 9
    assert hip_lib.occd_wino_conv3x3_fwd(ctypes.byref(w), None) == -1                  # act code
    assert hip_lib.occd_wino_pack_weights(None, None, None, 8, 8, None) == -1
    assert hip_lib.occd_pw_packed_floats(48, 288) == 36 * 2 * 256
    assert hip_lib.occd_pw_pack_weights(None, None, None, 8, 8, None) == -1
    a = hip.PwArgs()
    assert hip_lib.occd_pw_conv_fwd(ctypes.byref(a), None) == -1
    a.x = a.wpk = a.y = ptr
    a.batch, a.cin, a.cout, a.N = 1, 8, 8, 16
    a.tile_hint = 13
    assert hip_lib.occd_pw_conv_fwd(ctypes.byref(a), None) == -1                       # unknown variant (1..6 K11, 7..12 K11s)
    a.tile_hint, a.out_nhwc_cs = 0, 4
    assert hip_lib.occd_pw_conv_fwd(ctypes.byref(a), None) == -1                       # NHWC row shorter than Cout
    assert hip_lib.occd_dwconv2d_pool_blocks(185, 610) == (185 * 153 + 255) // 256
    assert hip_lib.occd_dwconv2d_pool_nchw(ptr, ptr, None, None, ptr, None, 1, 1, 4, 4, 3, 1, 1, 1, 4, 4, 0, 0, None) == -1
    assert hip_lib.occd_dwconv2d_pool_nchw(ptr, ptr, None, None, ptr, ptr, 1, 1, 4, 4, 3, 1, 1, 1, 4, 4, 0, 15, None) == -1   # plane stride < H * W
    assert hip_lib.occd_se_gate(None, None, None, None, None, None, None, 1, 8, 2, 1, 16, None) == -1
    assert hip_lib.occd_lift_bwd(None, None) == -1
    q = hip.LiftBwdArgs()
    assert hip_lib.occd_lift_bwd(ctypes.byref(q), None) == -1
    assert hip_lib.occd_softmax_nchw(None, None, 1, 4, 8, None) == -1


def test_gemm_entry_point_validates_kernel_hints(hip_lib):
    """occd_gemm_f32x3: host-side checks around the kernel hints (no launch for invalid arguments) -- hint 8 (K16p, the
    panel-stationary kernel) needs the pre-split A image, a plain epilogue and a K whose 32-column panel fits LDS."""
    from occdepth_amd import hip
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63            # 64-byte aligned dummy address (never dereferenced: every call is rejected)
    q = hip.GemmArgs()
    q.A = q.B = q.C = ptr
    q.M, q.N, q.K, q.batch = 256, 64, 64, 1
    q.lda, q.ldb, q.ldc = 64, 64, 64
    for hint in (-1, 9):
        q.tile_hint = hint
        assert hip_lib.occd_gemm_f32x3(ctypes.byref(q), None) == -1
    q.tile_hint = 8                                      # float32 A: not the panel kernel's operand
    q.pre = 0
    assert hip_lib.occd_gemm_f32x3(ctypes.byref(q), None) == -1
    q.pre, q.K, q.lda = 1, 856, 856                      # 864 k x 192 B > 160 KB of LDS
    assert hip_lib.occd_gemm_f32x3(ctypes.byref(q), None) == -1
    q.K, q.lda, q.res = 64, 64, ptr                      # a residual operand: K16's epilogue, not K16p's
    assert hip_lib.occd_gemm_f32x3(ctypes.byref(q), None) == -1
    q.res, q.act_a = None, 1                             # sigmoid on A needs the float32 operand
    assert hip_lib.occd_gemm_f32x3(ctypes.byref(q), None) == -1
    q.act_a, q.K = 0, 60                                 # K % 8
    assert hip_lib.occd_gemm_f32x3(ctypes.byref(q), None) == -1


# ----------------------------------------------------------------------------- the header parser, on small strings
SMALL = """
/* a comment with a ; and a { in it */
#ifndef SMALL_H
#define SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define OCCD_MAX_VIEWS 4
#define OCCD_MAX_SCALES 3
#define OCCD_EINVAL (-1)   /* parenthesised */
#define OCCD_HEX 0x10
typedef struct occd_inner {
    float* out;
    double origin[3];
    char tag[8];
} occd_inner;
typedef struct occd_outer {
    const float* in;                                   /* `in` is a Python keyword */
    const float* feat[OCCD_MAX_SCALES][OCCD_MAX_VIEWS];
    int32_t feat_h[OCCD_MAX_SCALES], feat_w[OCCD_MAX_SCALES];
    float scale_const;
    const uint8_t* const_ptr, *second;
    int64_t rows;
    uint32_t need;
    occd_inner inner;
    occd_inner two[2];
    const occd_inner* table;
} occd_outer;
int occd_version(void);
const char* occd_text(int code);
int64_t occd_run(const occd_outer* a, int32_t n, double x, void** created, void* const* boxes, const void* h,
                 int32_t* status, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SMALL_H */
"""


def small():
    from occdepth_amd import abi
    return abi.parse(SMALL)


def test_parser_constants():
    consts, _, _ = small()
    assert consts == {"OCCD_MAX_VIEWS": 4, "OCCD_MAX_SCALES": 3, "OCCD_EINVAL": -1, "OCCD_HEX": 16}


def test_parser_scalar_pointer_and_array_fields():
    from ctypes import c_char, c_double, c_float, c_int32, c_int64, c_uint32, c_void_p
    _, structs, _ = small()
    assert list(structs) == ["occd_inner", "occd_outer"]
    assert structs["occd_inner"]._fields_ == [("out", c_void_p), ("origin", c_double * 3), ("tag", c_char * 8)]
    f = dict(structs["occd_outer"]._fields_)
    assert [n for n, _ in structs["occd_outer"]._fields_] == [
        "inp", "feat", "feat_h", "feat_w", "scale_const", "const_ptr", "second", "rows", "need", "inner", "two", "table"]
    assert f["inp"] is c_void_p and f["rows"] is c_int64 and f["need"] is c_uint32
    assert f["scale_const"] is c_float                 # a name that contains `const` keeps it
    assert f["const_ptr"] is c_void_p and f["second"] is c_void_p
    assert f["feat_h"] is c_int32 * 3 and f["feat_w"] is c_int32 * 3      # two declarators, one base type
    assert f["table"] is c_void_p                      # pointer fields hold raw addresses, whatever they point to


def test_parser_2d_array_of_pointers_takes_integers():
    from ctypes import c_void_p
    _, structs, _ = small()
    assert dict(structs["occd_outer"]._fields_)["feat"] is (c_void_p * 4) * 3
    a = structs["occd_outer"]()
    a.feat[2][3] = 0x1000
    a.inp = 0x2000
    assert a.feat[2][3] == 0x1000 and a.feat[0][0] is None and a.inp == 0x2000
    with pytest.raises(IndexError):
        a.feat[3][0] = 1


def test_parser_nested_struct():
    _, structs, _ = small()
    inner, outer = structs["occd_inner"], structs["occd_outer"]
    f = dict(outer._fields_)
    assert f["inner"] is inner and f["two"] is inner * 2
    assert outer.two.offset - outer.inner.offset == ctypes.sizeof(inner) == 8 + 24 + 8


def test_parser_prototypes():
    from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_void_p
    _, structs, exports = small()
    assert list(exports) == ["occd_version", "occd_text", "occd_run"]
    assert exports["occd_version"] == (c_int32, [])                       # (void)
    assert exports["occd_text"] == (c_char_p, [c_int32])                  # const char* return
    assert exports["occd_run"] == (c_int64, [POINTER(structs["occd_outer"]), c_int32, c_double, POINTER(c_void_p),
                                             POINTER(c_void_p), c_void_p, c_void_p, c_void_p])


@pytest.mark.parametrize("name,text", [
    ("unknown type", "typedef struct occd_t { size_t n; } occd_t;"),
    ("unknown parameter type", "int occd_f(unsigned n);"),
    ("function-pointer field", "typedef struct occd_t { int (*cb)(int); } occd_t;"),
    ("bitfield", "typedef struct occd_t { int32_t a : 3; } occd_t;"),
    ("extent that is no integer", "#define OCCD_N (2 * 3)\ntypedef struct occd_t { int32_t a[OCCD_N]; } occd_t;"),
    ("extent that is not defined", "typedef struct occd_t { int32_t a[OCCD_N]; } occd_t;"),
    ("leftover text", "int occd_f(void);\nstray words\nint occd_g(void);"),
    ("unterminated declaration", "int occd_f(void);\nint occd_g(void)"),
    ("function body", "int occd_f(void) { return 0; }"),
    ("empty parameter list", "int occd_f();"),
    ("anonymous struct", "typedef struct { int32_t a; } occd_t;"),
    ("nested definition", "typedef struct occd_t { struct { int32_t a; } s; } occd_t;"),
    ("field without a name", "typedef struct occd_t { int32_t; } occd_t;"),
    ("void field", "typedef struct occd_t { void a; } occd_t;"),
    ("array parameter", "int occd_f(int32_t a[3]);"),
    ("function-like macro", "#define OCCD_F(x) x"),
    ("conditional", "#if 1\nint occd_f(void);\n#endif"),
    ("line comment", "int occd_f(void); // no"),
    ("function declared twice", "int occd_f(void);\nint occd_f(void);"),
])
def test_parser_rejects(name, text):
    from occdepth_amd import abi
    with pytest.raises(abi.HeaderError):
        abi.parse(text)


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    """Without the header there is no binding: importing abi raises and names the path (run on a copy of the module,
    so the loaded binding is left alone)."""
    import importlib.util
    from occdepth_amd import abi
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    (pkg / "abi.py").write_text(open(abi.__file__).read())
    spec = importlib.util.spec_from_file_location("abi_without_header", str(pkg / "abi.py"))
    with pytest.raises(RuntimeError, match="occdepth_amd.h is missing"):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))


def test_derived_prototypes_spot_pinned():
    """A handful of prototypes of the real header against literals: a parser regression shows as a readable diff."""
    from ctypes import POINTER, c_float, c_int32, c_int64, c_void_p
    from occdepth_amd import abi, hip
    assert hip.EXPORTS is abi.EXPORTS and hip.ABI_VERSION == abi.ABI_VERSION == abi.CONSTANTS["OCCD_ABI_VERSION"]
    assert abi.EXPORTS["occd_abi_version"] == (c_int32, [])
    assert abi.EXPORTS["occd_conv3d_fwd"] == (c_int32, [POINTER(hip.Conv3dArgs), c_void_p])
    assert abi.EXPORTS["occd_bn_fwd_small_xchg"] == (
        c_int32, [POINTER(hip.BnArgs), c_void_p, c_float, c_float] + [c_void_p] * 9 +
        [POINTER(c_void_p), c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p])
    assert abi.EXPORTS["occd_gemm_f32x3_splitk"] == (
        c_int32, [POINTER(hip.GemmArgs), c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p])
    assert hip.Conv3dArgs._fields_[0] == ("inp", c_void_p) and hip.Conv3dArgs is abi.STRUCTS["occd_conv3d_args"]
    assert dict(hip.LiftArgs._fields_)["feat"] is (c_void_p * hip.MAX_VIEWS) * hip.MAX_SCALES
