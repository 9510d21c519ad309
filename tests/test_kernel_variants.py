"""Kernel variants that a host rule selects and that no other test shape reaches.

Several entry points pick a template instantiation or a fallback kernel from their arguments: the table lift and its backward
(`lift_p1_kernel<LPV, V, P2>`, `lift_p1_bwd_kernel<LPV, V>`, csrc/lift.hip), the cascade tail (`cascade_tail_lds_kernel<NG>` /
`cascade_tail_kernel<NG>`, csrc/nchw2d.hip), the depthwise forward (`dwconv2d_direct_kernel` once the staged kernel's LDS tile
passes 48 KiB) and the depthwise backward kernels.  The case tables below name the variant each case is meant to launch;
`test_case_tables_select_the_variants_they_name` restates every host rule as a Python predicate (with the source line it
mirrors, which must still be in the source) and proves the tables, on the CPU.  The GPU tests compare every variant with a
float64 reference of the same operation.

Bounds.  The lift keeps the bounds of tests/test_lift_autograd.py (1e-5 forward, 1e-4 gradients, of the tensor maximum); the
entries of the zeroed feature rows, whose gradient is the b^ / eps term of the clamped cosine (~1e8), are compared with their
own row's maximum and everything else with the maximum of the rest.  The cascade tail is bounded by twice the error of the same
formula in float32 ATen on the GPU (the pattern of tests/test_clip_adamw_gpu.py).  The depthwise tests keep the bounds of
tests/test_dwconv_staged.py and of test_depthwise_autograd_gpu (tests/test_pw_gemm.py)."""
import ctypes
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

import emu
from test_dwconv_staged import NAMES as DW_NAMES, _inputs as dw_inputs, geometries as dw_geometries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _ceil_div(a, b):
    return -(-a // b)


def _round_up(a, m):
    return _ceil_div(a, m) * m


def _pow2(v):
    return v > 0 and v & (v - 1) == 0


# ------------------------------------------------------------------------------------------------------- the host rules
# Each predicate restates one rule of the library; RULES lists the source text it mirrors (checked to be still there).
RULES = [
    ("lift.hip", "const int lpv = need <= 8 ? 8 : need <= 16 ? 16 : need <= 32 ? 32 : 64;"),      # occd_lift_fwd, occd_lift_bwd
    ("lift.hip", "if (!all || p.bc_shift < 0 || p.c_shift < 0) p.bc_shift = p.c_shift = -1;"),    # P2
    ("lift.hip", "if (p.a.xcd_mode == 2 && ((long)a->dimB * a->dimC * lpv) % 2048 != 0) p.a.xcd_mode = 0;"),
    ("lift.hip", "if (p.a.xcd_mode == 2 && threads % 256 != 0) p.a.xcd_mode = 0;"),
    ("nchw2d.hip", "if (Z <= 64 && X <= 65535 && batch <= 65535) {"),                             # occd_cascade_tail_fwd
    ("nchw2d.hip", "const int TY = 256 / Z;"),
    ("nchw2d.hip", "if (ng <= 3) OCCD_TAIL_LDS(3);"),
    ("nchw2d.hip", "else if (ng <= 5) OCCD_TAIL_LDS(5);"),
    ("nchw2d.hip", "if (ng <= 3) OCCD_TAIL(3);"),
    ("nchw2d.hip", "else if (ng <= 5) OCCD_TAIL(5);"),
    ("nchw2d.hip", "int dmax = (255 + wq - 1) / wq;"),                                            # dwconv_launch
    ("nchw2d.hip", "const size_t lds = (size_t)(dmax * stride + k) * wp * sizeof(float);"),
    ("nchw2d.hip", "if (lds <= 48 * 1024) {"),
    ("dwconv_stage.h", "return 4 * (wq - 1) * stride + 4 * span4;"),                              # dw_tile_wp
    ("nchw2d.hip", "long chunks = ((long)batch * Ho * Wo + 256 * 16 - 1) / (256 * 16);"),        # occd_dwconv2d_bwd_weight_nchw
    ("nchw2d.hip", "if (chunks > 64) chunks = 64;"),
]


def lift_lpv(cs):
    """Lanes per voxel from the row width in floats (csrc/lift.hip, occd_lift_fwd and occd_lift_bwd: `need = out_cs / 4`)."""
    need = cs // 4
    return 8 if need <= 8 else 16 if need <= 16 else 32 if need <= 32 else 64


def lift_row_widths(C):
    """(forward, backward) row width the wrappers allocate: Vox.empty rounds the forward's rows up to 8 floats
    (occdepth_amd/hip.py), _LiftFn.backward pads the upstream gradient to 4 (occdepth_amd/lift_autograd.py)."""
    return _round_up(C, 8), _round_up(C, 4)


def lift_p2(scene, scales):
    """Shift form of the index arithmetic (csrc/lift.hip, occd_lift_fwd: every scale divisor, dimB * dimC and dimC a power of 2)."""
    return all(_pow2(s) for s in scales) and _pow2(scene[1] * scene[2]) and _pow2(scene[2])


def lift_xcd_mode(scene, lpv, asked):
    """The placement mode that runs (csrc/lift.hip, occd_lift_fwd): mode 2 needs whole slabs of 8 workgroups."""
    N = scene[0] * scene[1] * scene[2]
    if asked == 2 and ((scene[1] * scene[2] * lpv) % 2048 != 0 or (N * lpv) % 256 != 0):
        return 0
    return asked


def tail_route(Z, nbr):
    """(form, TY, NG) of occd_cascade_tail_fwd (csrc/nchw2d.hip): the LDS form iff Z <= 64, NG from ceil(nbr / 4)."""
    ng = _ceil_div(nbr, 4)
    NG = 3 if ng <= 3 else 5 if ng <= 5 else 8
    return ("lds", 256 // Z, NG) if Z <= 64 else ("generic", None, NG)


def dw_tile_bytes(H, W, k, s):
    """LDS tile of the staged depthwise kernel (csrc/nchw2d.hip, dwconv_launch; dw_tile_wp: csrc/dwconv_stage.h)."""
    Ho, Wo = _ceil_div(H, s), _ceil_div(W, s)
    wq, span4 = (Wo + 3) // 4, ((3 * s + k) + 3) // 4
    wp = 4 * (wq - 1) * s + 4 * span4
    dmax = min((255 + wq - 1) // wq, Ho - 1)
    return (dmax * s + k) * wp * 4


def dw_route(H, W, k, s):
    return "direct" if dw_tile_bytes(H, W, k, s) > 48 * 1024 else "staged"


def wgrad_chunks(B, Ho, Wo):
    """(grid.x of dwconv2d_bwd_weight_kernel, the same before the cap): csrc/nchw2d.hip, occd_dwconv2d_bwd_weight_nchw."""
    raw = _ceil_div(B * Ho * Wo, 4096)
    return min(64, raw), raw


# ------------------------------------------------------------------------------------------------------- the case tables
IMAGE = (17, 29)                                                       # (H, W)
LIFT_GRIDS = {"p2": ((8, 8, 4), (1, 2, 4, 8)),                         # every divisor a power of two: lift_p1_kernel<.., true>
              "div": ((6, 5, 7), (1, 3))}                              # integer divisions; N * LPV is no multiple of 256
# C -> (LPV, lanes of a voxel group that hold channels): LPV 8, a ragged 16, a ragged 32, a full 32, a ragged 64, a full 64
LIFT_LANES = {8: (8, 2), 36: (16, 9), 68: (32, 17), 128: (32, 32), 132: (64, 33), 256: (64, 64)}
# (grid, C, V, B, with depth volume): every (C, V) pair on both grids
LIFT_CASES = [(g, C, V, 2 if (i + j) % 5 == 0 else 1, (i + j) % 2 == 0)
              for i, (C, V) in enumerate(itertools.product(LIFT_LANES, (1, 2, 3, 4))) for j, g in enumerate(LIFT_GRIDS)]
# workgroup placement, forward only: (scene, C, what the case is for)
XCD_CASES = [((4, 16, 16), 32, "mode2"), ((4, 16, 32), 32, "mode2-permutes"), ((6, 5, 7), 128, "mode1-ragged")]

# (B, X, Y, Z, nbr, part_cs, occ_off) -> (form, TY, NG) it must launch
TAIL_CASES = [
    ((1, 3, 9, 32, 20, 24, 20), ("lds", 8, 5)),                        # two y-tiles, the second with one live row
    ((2, 2, 5, 60, 12, 16, 12), ("lds", 4, 3)),                        # 240 live threads of 256
    ((1, 2, 3, 24, 27, 32, 28), ("lds", 10, 8)),                       # NG = 8 and the scalar tail stores
    ((1, 2, 5, 64, 20, 24, 20), ("lds", 4, 5)),                        # the largest Z of the LDS form
    ((1, 1, 1, 1, 1, 12, 2), ("lds", 256, 3)),                         # one voxel: every tap but the centre is padding
    ((1, 2, 3, 65, 20, 24, 20), ("generic", None, 5)),                 # the smallest Z of the generic form
    ((2, 3, 2, 96, 12, 16, 12), ("generic", None, 3)),
    ((1, 2, 2, 72, 27, 32, 28), ("generic", None, 8)),
]
# Accepted before, rejected now: a variant loads 4 * NG floats of every part row.  (1, 1, 1, 1, 1, 4, 2) is the one-voxel
# case with the narrowest row that ceil4(nbr) allows: NG = 3 reads 12 floats of its 4, so it runs above with part_cs = 12.
TAIL_TOO_NARROW = [(1, 1, 1, 1, 13, 16, 14), (1, 1, 1, 1, 1, 4, 2), (1, 2, 2, 8, 21, 24, 22), (1, 1, 1, 1, 13, 16, 12)]

# depthwise forward (B, C, H, W, k, stride) -> bytes of the staged kernel's tile
DW_DIRECT = {(1, 2, 3, 2100, 5, 1): 50496, (1, 2, 3, 3100, 3, 1): 49664, (1, 2, 5, 1800, 5, 2): 64944, (1, 2, 5, 2500, 3, 2): 50160}
DW_STAGED_PARTNER = {(1, 2, 3, 2000, 5, 1): 48096}
DW_FORWARD = list(DW_DIRECT) + list(DW_STAGED_PARTNER)

# depthwise backward: the forward's edge geometries, then the 64-chunk cap and the bottom/right-only pad
DW_BWD_EDGES = [(name, k, stride) for name in DW_NAMES for k in (3, 5) for stride in (1, 2)]
DW_BWD_CAP = (1, 2, 520, 520, 3, 1)
DW_BWD_PAD_BR = (2, 3, 6, 10, 3, 2)


# ------------------------------------------------------------------------------------------------------- lift: inputs, reference
def lift_inputs(case):
    """Feature maps per scale and view, pixel tables, field-of-view masks (probability 0.5), depth volume, upstream gradient.
    Degenerate rows: the row of view 0 at pixel (0, 0) and the rows of every view at pixel (1, 1) are zero at every scale;
    voxels 0..4 look at (0, 0) and 5..9 at (1, 1) in all views, so pairs (zero row, row) and (zero row, zero row) occur."""
    grid, C, V, B, with_depth = case
    scene, scales = LIFT_GRIDS[grid]
    H, W = IMAGE
    g = torch.Generator().manual_seed(1000 * C + 10 * V + B + len(scales))
    N = scene[0] * scene[1] * scene[2]
    feats = [[torch.randn(B, C, _ceil_div(H, s), _ceil_div(W, s), generator=g) for _ in range(V)] for s in scales]
    for per in feats:
        per[0][:, :, 0, 0] = 0
        for f in per:
            f[:, :, 1, 1] = 0
    px = torch.randint(0, W, (B, V, N, 1, 1), generator=g)
    py = torch.randint(0, H, (B, V, N, 1, 1), generator=g)
    pix = torch.cat([px, py], -1)
    fov = torch.rand(B, V, N, 1, generator=g) < 0.5
    pix[:, :, 0:5] = 0
    pix[:, :, 5:10] = 1
    fov[:, :, 0:10] = True
    depth = torch.rand(B, 1, *scene, generator=g) if with_depth else None
    R = torch.randn(B, C, *scene, generator=g)
    return feats, pix, fov, depth, R


def lift_reference(case, inputs, dtype=torch.float64, device="cpu"):
    """The reference-structure ATen graph of tests/test_lift_autograd.py (per sample and scale `SFA._forward_autograd`, then
    `* depth * 100`) and its autograd gradients, in `dtype` on `device`; results as float64 CPU tensors."""
    from occdepth_amd.models.SFA import SFA
    grid, C, V, B, with_depth = case
    scene, scales = LIFT_GRIDS[grid]
    feats, pix, fov, depth, R = inputs
    feats = [[f.to(device=device, dtype=dtype).requires_grad_(True) for f in per] for per in feats]
    pix, fov = pix.to(device), fov.to(device)
    d = depth.to(device=device, dtype=dtype).requires_grad_(True) if with_depth else None
    sfa = SFA(scene, "kitti", 1)
    outs = []
    for b in range(B):
        x3d = 0
        for si, s in enumerate(scales):
            x2d = torch.stack([feats[si][v][b] for v in range(V)])
            x3d = x3d + sfa._forward_autograd(x2d, torch.div(pix[b], s, rounding_mode="floor"), fov[b])
        outs.append(x3d)
    out = torch.stack(outs)
    if with_depth:
        out = out * d * 100
    (out * R.to(device=device, dtype=dtype)).sum().backward()
    return (out.detach().double().cpu(), [[f.grad.double().cpu() for f in per] for per in feats],
            d.grad.double().cpu() if with_depth else None)


def lift_kernels(case, inputs):
    """The HIP forward and its one-launch backward through occdepth_amd.lift_autograd; results as float64 CPU tensors."""
    from occdepth_amd import lift_autograd
    grid, C, V, B, with_depth = case
    scene, scales = LIFT_GRIDS[grid]
    feats, pix, fov, depth, R = inputs
    dev_feats = [[f.cuda().requires_grad_(True) for f in per] for per in feats]
    dev_depth = depth.cuda().requires_grad_(True) if with_depth else None
    assert lift_autograd.usable(dev_feats, pix.cuda())
    out = lift_autograd.lift_scales_autograd(dev_feats, list(scales), pix.cuda(), fov.cuda(), scene, 1, "kitti",
                                             depth_scale=dev_depth, scale_const=100.0)
    (out * R.cuda()).sum().backward()
    return (out.detach().double().cpu(), [[f.grad.double().cpu() for f in per] for per in dev_feats],
            dev_depth.grad.double().cpu() if with_depth else None)


def lift_errors(got, ref):
    """{"out", "gfeat", "grow", "gdepth"}: forward and depth-gradient error over the tensor maximum; feature-gradient error
    outside the zeroed rows over the maximum of those entries (largest over scales and views); and for every zeroed row
    its error over the row's own maximum (largest over the rows; a row the reference leaves at zero must be zero)."""
    (out, gf, gd), (rout, rgf, rgd) = got, ref
    assert out.shape == rout.shape and torch.isfinite(rout).all() and torch.isfinite(out).all()
    err = {"out": float((out - rout).abs().max() / rout.abs().max()), "gfeat": 0.0, "grow": 0.0, "gdepth": 0.0}
    for per, rper in zip(gf, rgf):
        for v, (g, r) in enumerate(zip(per, rper)):
            assert g.shape == r.shape and torch.isfinite(r).all() and torch.isfinite(g).all()
            zeroed = torch.zeros(r.shape[2:], dtype=torch.bool)
            zeroed[1, 1] = True
            zeroed[0, 0] = v == 0
            rest = ~zeroed
            err["gfeat"] = max(err["gfeat"], float((g - r)[:, :, rest].abs().max() / r[:, :, rest].abs().max()))
            for y, x in zeroed.nonzero().tolist():
                for b in range(r.shape[0]):
                    top = float(r[b, :, y, x].abs().max())
                    e = float((g - r)[b, :, y, x].abs().max())
                    err["grow"] = max(err["grow"], e / top if top > 0 else (0.0 if e == 0 else float("inf")))
    if rgd is not None:
        assert gd.shape == rgd.shape
        err["gdepth"] = float((gd - rgd).abs().max() / rgd.abs().max())
    return err


def lift_view_counts(case, fov):
    """(voxels no view sees, voxels exactly one view sees)."""
    seen = fov[..., 0].sum(1)
    return int((seen == 0).sum()), int((seen == 1).sum())


# ------------------------------------------------------------------------------------------------------- 0. the tables (CPU)
def test_case_tables_select_the_variants_they_name(hip_lib):
    for name, text in RULES:                                           # the rules restated above are still the library's
        with open(os.path.join(ROOT, "occdepth_amd", "csrc", name)) as f:
            assert text in f.read(), (name, text)

    # ---- lift: (LPV, V, P2), forward and backward, every pair on both grids
    assert lift_p2(*LIFT_GRIDS["p2"]) and not lift_p2(*LIFT_GRIDS["div"])
    seen = set()
    for case in LIFT_CASES:
        grid, C, V, B, with_depth = case
        scene, scales = LIFT_GRIDS[grid]
        lpv, lanes = LIFT_LANES[C]
        fwd_cs, bwd_cs = lift_row_widths(C)
        assert lift_lpv(fwd_cs) == lift_lpv(bwd_cs) == lpv and C == 4 * lanes and lanes <= lpv and (C == 8 or lanes > lpv // 2)
        N = scene[0] * scene[1] * scene[2]
        if grid == "div":
            assert (N * lpv) % 256 != 0                                # the last workgroup is ragged
        feats, pix, fov, depth, R = lift_inputs(case)
        none, one = lift_view_counts(case, fov)
        assert none > 0 and one > 0, case
        assert bool(fov[:, :, :10].all()) and int(pix[:, :, :5].abs().max()) == 0 and bool((pix[:, :, 5:10] == 1).all())
        assert all(float(per[0][:, :, 0, 0].abs().max()) == 0 and all(float(f[:, :, 1, 1].abs().max()) == 0 for f in per)
                   for per in feats)
        assert max(f.numel() for per in feats for f in per) < 300000
        seen.add((grid, lpv, V, B, with_depth))
    for grid in LIFT_GRIDS:
        assert {(l, v) for g, l, v, _, _ in seen if g == grid} == set(itertools.product((8, 16, 32, 64), (1, 2, 3, 4)))
        assert {(b, d) for g, _, _, b, d in seen if g == grid} == {(1, False), (1, True), (2, False), (2, True)}
    assert {lanes == lpv for lpv, lanes in LIFT_LANES.values()} == {True, False}
    for scene, C, what in XCD_CASES:
        lpv = lift_lpv(lift_row_widths(C)[0])
        nwg = _ceil_div(scene[0] * scene[1] * scene[2] * lpv, 256)
        if what.startswith("mode2"):
            assert lpv == 8 and lift_xcd_mode(scene, lpv, 2) == 2
            per_xcd = scene[1] * scene[2] * lpv // 256 // 8            # runs of xcd_slab_interleave: 1 is the identity
            assert per_xcd == (2 if what == "mode2-permutes" else 1)
        else:
            assert nwg % 8 != 0 and nwg > 8 and lift_xcd_mode(scene, lpv, 2) == 0 and lift_xcd_mode(scene, lpv, 1) == 1

    # ---- cascade tail
    routes = set()
    for (B, X, Y, Z, nbr, part_cs, occ_off), claim in TAIL_CASES:
        assert tail_route(Z, nbr) == claim
        assert 4 * claim[2] <= part_cs and occ_off % 2 == 0 and occ_off + 2 <= part_cs and B * X * Y * Z * part_cs < 50000
        routes.add((claim[0], claim[2]))
    assert routes == set(itertools.product(("lds", "generic"), (3, 5, 8)))
    (_, _, Y, Z, nbr, _, _), (_, TY, _) = TAIL_CASES[0]
    assert _ceil_div(Y, TY) == 2 and Y % TY == 1
    (_, _, Y, Z, _, _, _), (_, TY, _) = TAIL_CASES[1]
    assert TY * Z == 240 and Y % TY != 0
    assert all(nbr % 4 != 0 for (_, _, _, _, nbr, _, _), claim in TAIL_CASES if claim[2] == 8)
    assert {Z for (_, _, _, Z, _, _, _), _ in TAIL_CASES} >= {64, 65}
    for B, X, Y, Z, nbr, part_cs, occ_off in TAIL_TOO_NARROW:          # valid by every other rule of the entry point
        assert _round_up(nbr, 4) <= part_cs < 4 * tail_route(Z, nbr)[2] and occ_off % 2 == 0 and occ_off + 2 <= part_cs

    # ---- depthwise forward: the two sides of the 48 KiB branch
    for table, route in ((DW_DIRECT, "direct"), (DW_STAGED_PARTNER, "staged")):
        for (B, C, H, W, k, s), nbytes in table.items():
            assert dw_tile_bytes(H, W, k, s) == nbytes and dw_route(H, W, k, s) == route
            Ho, Wo = _ceil_div(H, s), _ceil_div(W, s)
            items = Ho * ((Wo + 3) // 4)
            assert items > 512 and items % 256 != 0                    # several blocks, the last one ragged
            assert hip_lib.occd_dwconv2d_pool_blocks(Ho, Wo) == _ceil_div(items, 256)
            assert (H * W) % 32 != 0                                   # the padded pitch differs from the dense one
    for stride in (1, 2):                                              # ... and everything tested before is staged
        for B, C, H, W in dw_geometries(stride).values():
            assert all(dw_route(H, W, k, stride) == "staged" for k in (3, 5))

    # ---- depthwise weight gradient: the cap of the grid
    for shape, capped in [(DW_BWD_CAP, True), (DW_BWD_PAD_BR, False)]:
        B, C, H, W, k, s = shape
        Ho, Wo = _ceil_div(H, s), _ceil_div(W, s)
        chunks, raw = wgrad_chunks(B, Ho, Wo)
        assert (raw > 64) == capped and chunks == min(raw, 64)
        assert hip_lib.occd_dwconv2d_bwd_weight_workspace_floats(B, C, k, Ho, Wo) == C * chunks * k * k
    B, C, H, W, k, s = DW_BWD_PAD_BR
    assert s == 2 and H % 2 == 0 and W % 2 == 0 and k == 3             # pad_h = pad_w = 1: top / left get 1 // 2 = 0
    assert max((_ceil_div(H, s) - 1) * s + k - H, 0) // 2 == 0 and max((_ceil_div(W, s) - 1) * s + k - W, 0) // 2 == 0


def test_cascade_tail_rejects_rows_narrower_than_its_loads_cpu(hip_lib):
    """Host-side check only (no launch for invalid arguments): `part_cs` must cover the 4 * NG floats that the variant loads
    from every row, not just ceil4(nbr): nbr = 13 takes NG = 5 and reads 20 floats, 16 bytes past a 16-float last row."""
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    for B, X, Y, Z, nbr, part_cs, occ_off in TAIL_TOO_NARROW:
        assert hip_lib.occd_cascade_tail_fwd(p, p, p, B, X, Y, Z, part_cs, occ_off, _round_up(nbr, 4), nbr, None) == -1
    assert hip_lib.occd_cascade_tail_fwd(p, p, p, 1, 1, 1, 1, 16, 14, 12, 13, None) == -1        # (nbr > out_cs, as before)


# ------------------------------------------------------------------------------------------------------- 1. lift (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("case", LIFT_CASES, ids=lambda c: "%s-C%d-V%d-B%d-%s" % (c[0], c[1], c[2], c[3], "depth" if c[4] else "nodepth"))
def test_lift_variants_match_the_float64_graph(case, hip_lib):
    """lift_p1_kernel<LPV, V, P2> and lift_p1_bwd_kernel<LPV, V> for LPV in {8, 16, 32, 64} x V in {1..4} x both index forms,
    with voxels that no view and that exactly one view sees, and with zero feature rows under the 1e-8 clamp of the cosine.

    The bounds are those of tests/test_lift_autograd.py.  Measured on an MI355X, largest over the 48 cases, kernel / the same
    ATen graph in float32 on the GPU: forward 1.5e-7 / 1.5e-7, feature gradients 2.8e-7 / 2.3e-7, zeroed rows (gradients of
    ~1e8, over their own maximum; float atomics, so the last digits vary) 6.5e-6 / 4.4e-6, depth gradient 1.5e-7 / 2.0e-7."""
    inputs = lift_inputs(case)
    none, one = lift_view_counts(case, inputs[2])
    assert none > 0 and one > 0
    err = lift_errors(lift_kernels(case, inputs), lift_reference(case, inputs))
    print("lift", case, err)
    assert err["out"] < 1e-5, err
    assert err["gfeat"] < 1e-4 and err["grow"] < 1e-4 and err["gdepth"] < 1e-4, err


def _lift_forward(feats, scales, pix, fov, scene, depth, xcd_mode):
    """occd_lift_fwd through hip.lift into a NaN-prefilled voxel buffer, with the placement mode asked for."""
    from occdepth_amd import hip
    from occdepth_amd.models.SFA import pixel_rows, voxel_layout
    n_dims, out_dims, strides = voxel_layout(scene, 1, "kitti")
    rows = [[pixel_rows(f) for f in per] for per in feats]
    B, C = feats[0][0].shape[:2]
    out = hip.Vox(torch.full((B,) + tuple(out_dims) + (_round_up(C, 8),), NAN, device="cuda"), C)
    hip.lift(rows, list(scales), pix, fov, n_dims, strides, out, depth_scale=depth, scale_const=100.0, xcd_mode=xcd_mode)
    return out.buf


@pytest.mark.gpu
@pytest.mark.parametrize("scene,C,what", XCD_CASES, ids=[c[2] for c in XCD_CASES])
def test_lift_workgroup_placement_changes_no_value(scene, C, what, hip_lib):
    """xcd_mode 1 (xcd_remap) and 2 (xcd_slab_interleave) only permute the workgroups: every voxel row is written, once,
    with the same bits as in dispatch order.  Where mode 2 is not eligible the library runs mode 0."""
    g = torch.Generator().manual_seed(C + scene[2])
    H, W = IMAGE
    scales, V, B = (1, 2, 4, 8), 2, 2
    N = scene[0] * scene[1] * scene[2]
    feats = [[torch.randn(B, C, _ceil_div(H, s), _ceil_div(W, s), generator=g).cuda() for _ in range(V)] for s in scales]
    pix = torch.cat([torch.randint(0, W, (B, V, N, 1, 1), generator=g), torch.randint(0, H, (B, V, N, 1, 1), generator=g)], -1).cuda()
    fov = (torch.rand(B, V, N, 1, generator=g) < 0.7).cuda()
    depth = torch.rand(B, N, generator=g).cuda()
    base = _lift_forward(feats, scales, pix, fov, scene, depth, 0)
    assert torch.isfinite(base).all() and float(base.abs().max()) > 0
    for mode in (1, 2):
        assert torch.equal(_lift_forward(feats, scales, pix, fov, scene, depth, mode), base), mode


# ------------------------------------------------------------------------------------------------------- 2. cascade tail (GPU)
def _tail_inputs(case):
    B, X, Y, Z, nbr, part_cs, occ_off = case
    g = torch.Generator().manual_seed(100 * Z + nbr)
    part = torch.randn(B, X, Y, Z, part_cs, generator=g)
    part[..., occ_off:occ_off + 2] *= 4                                # the 2-way softmax saturates on some voxels
    return part, torch.randn(nbr, 2, 3, 3, 3, generator=g) * 0.3


def _tail_formula(part, wn, occ_off, nbr):
    """The header's formula in the dtype and on the device of its operands: softmax of the two occupancy logits, 3x3x3
    zero-padded convolution with wn, plus part[..., :nbr]."""
    soft = F.softmax(part[..., occ_off:occ_off + 2], dim=-1).permute(0, 4, 1, 2, 3)        # (as emu.cascade_tail: a strided view)
    if soft.is_contiguous():                                           # one voxel: the view's strides fit either memory format,
        soft = soft.clone(memory_format=torch.contiguous_format)       # and MIOpen refuses a one-filter weight in channels-last
    return F.conv3d(soft, wn, None, padding=1).permute(0, 2, 3, 4, 1) + part[..., :nbr]


def tail_errors(case, out_extra=0, tail_floats=64):
    """(kernel error, float32 ATen error on the GPU), both against the float64 formula on the CPU, over the tensor maximum.
    The entry point writes into a NaN-prefilled buffer with `tail_floats` more floats after the last row: lanes
    [nbr, out_cs) and the tail must still be NaN afterwards."""
    from occdepth_amd import hip
    B, X, Y, Z, nbr, part_cs, occ_off = case
    part, wn = _tail_inputs(case)
    ref = _tail_formula(part.double(), wn.double(), occ_off, nbr)
    pd, wd = part.cuda(), wn.cuda()
    out_cs = _round_up(nbr, 4) + out_extra
    rows = B * X * Y * Z
    flat = torch.full((rows * out_cs + tail_floats,), NAN, device="cuda")
    code = hip.load().occd_cascade_tail_fwd(pd.data_ptr(), wd.data_ptr(), flat.data_ptr(), B, X, Y, Z, part_cs, occ_off,
                                            out_cs, nbr, torch.cuda.current_stream().cuda_stream)
    assert code == 0, code
    got = flat[:rows * out_cs].view(B, X, Y, Z, out_cs).cpu()
    assert torch.isnan(got[..., nbr:]).all() and torch.isnan(flat[rows * out_cs:]).all()
    assert torch.isfinite(got[..., :nbr]).all()
    yard = _tail_formula(pd, wd, occ_off, nbr).double().cpu()
    top = ref.abs().max()
    return float((got[..., :nbr].double() - ref).abs().max() / top), float((yard - ref).abs().max() / top)


@pytest.mark.gpu
@pytest.mark.parametrize("case,claim", TAIL_CASES, ids=["%s-ng%d-z%d" % (c[1][0], c[1][2], c[0][3]) for c in TAIL_CASES])
def test_cascade_tail_variants_match_the_float64_formula(case, claim, hip_lib):
    """cascade_tail_lds_kernel<3 | 5 | 8> and cascade_tail_kernel<3 | 5 | 8> against the header's formula in float64.  Only
    lanes [0, nbr) of a row are written; the first case has a whole float4 of pad lanes (out_cs = 24 for nbr = 20).

    Bound: twice the error of the same formula in float32 ATen on the GPU (emu.cascade_tail's expression), both over max |ref|.
    Measured on an MI355X, kernel / ATen, in the order of TAIL_CASES: 1.29e-7 / 1.56e-7, 1.24e-7 / 1.67e-7, 1.14e-7 / 2.16e-7,
    1.28e-7 / 1.57e-7, 6.09e-8 / 6.09e-8 (one voxel), 1.59e-7 / 1.43e-7, 1.15e-7 / 1.40e-7, 1.36e-7 / 1.15e-7: at most 1.19 x.
    (Fed a dense NCDHW copy of the softmax instead of emu's strided view, MIOpen takes another algorithm that errs 6.4e-8 -
    7.1e-8 on the 2nd to 4th case, half a unit in the last place of the largest value; the kernel is 1.75 - 1.98 x that.)"""
    err, yard = tail_errors(case, out_extra=4 if case == TAIL_CASES[0][0] else 0)
    print("cascade tail", case, claim, "kernel %.3e float32 ATen %.3e" % (err, yard))
    assert err <= 2 * yard, (err, yard)


# ------------------------------------------------------------------------------------------------------- 3. depthwise forward (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("shape", DW_FORWARD, ids=["%s-%dx%d-k%d-s%d" % (dw_route(*s[2:]), s[2], s[3], s[4], s[5]) for s in DW_FORWARD])
def test_dwconv_direct_kernel_and_its_staged_neighbour(shape, hip_lib):
    """Rows so wide that the staged kernel's tile passes 48 KiB run dwconv2d_direct_kernel<K, STRIDE>: plain, with the pooling
    partials (several 256-item blocks, the last one ragged: its dead lanes join the reduction) and on the padded plane pitch
    with NaN between the planes; one geometry just below the limit stays on the staged kernel.  Bounds and reference are
    those of test_dwconv_chunked_staging_gpu."""
    from occdepth_amd import hip
    B, C, H, W, k, stride = shape
    x, w, sc, sh = dw_inputs((B, C, H, W), k)
    y_ref, part_ref, plane = emu.dwconv2d_same_pool(x, w, sc, sh, stride, "swish")
    xd, wd, scd, shd = x.cuda(), w.cuda(), sc.cuda(), sh.cuda()
    xp = hip.padded_rows((B, C, H * W), "cuda")
    assert xp.stride(1) > H * W
    torch.as_strided(xp, (B, C, xp.stride(1)), (xp.stride(0), xp.stride(1), 1)).fill_(NAN)
    xp.copy_(xd.view(B, C, H * W))
    y0 = hip.dwconv2d_same(xd, wd, scd, shd, stride, "swish")
    y1, p1, n1 = hip.dwconv2d_same_pool(xd, wd, scd, shd, stride, "swish")
    y2, p2, n2 = hip.dwconv2d_same_pool(xp.view(B, C, H, W), wd, scd, shd, stride, "swish")
    nblk = hip_lib.occd_dwconv2d_pool_blocks(-(-H // stride), -(-W // stride))
    assert n1 == n2 == plane and p1.shape == p2.shape == (B * C, nblk) and nblk > 1
    for y in (y0, y1, y2):
        assert y.shape == y_ref.shape
        assert torch.allclose(y.cpu(), y_ref, rtol=1e-5, atol=1e-5), float((y.cpu() - y_ref).abs().max())
    for p in (p1, p2):
        assert torch.allclose(p.double().sum(1).cpu(), part_ref.double().sum(1), rtol=1e-5, atol=1e-5 * plane)
    # the three launches run the same arithmetic in the same order
    assert torch.equal(y0, y1) and torch.equal(y1, y2) and torch.equal(p1, p2)


# ------------------------------------------------------------------------------------------------------- 4. depthwise backward (GPU)
def _dw_autograd_against_float64(shape):
    """hip.dwconv2d_same_autograd (forward, dwconv2d_bwd_data_kernel, dwconv2d_bwd_weight_kernel) against the float64 ATen
    graph of test_depthwise_autograd_gpu: asymmetric SAME padding, 2e-5 of the tensor maximum for y, dx and dw."""
    from occdepth_amd import hip
    B, C, H, W, k, stride = shape
    x, w, _, _ = dw_inputs((B, C, H, W), k)
    Ho, Wo = -(-H // stride), -(-W // stride)
    R = torch.randn(B, C, Ho, Wo, generator=torch.Generator().manual_seed(H + 7 * W + k))
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ph, pw_ = max((Ho - 1) * stride + k - H, 0), max((Wo - 1) * stride + k - W, 0)
    ref = F.conv2d(F.pad(xd, [pw_ // 2, pw_ - pw_ // 2, ph // 2, ph - ph // 2]), wd, None, stride, 0, 1, C)
    (ref * R.double()).sum().backward()
    xc, wc = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    y = hip.dwconv2d_same_autograd(xc, wc, stride)
    (y * R.cuda()).sum().backward()
    for what, got, want in (("y", y, ref), ("dx", xc.grad, xd.grad), ("dw", wc.grad, wd.grad)):
        assert got.shape == want.shape, what
        err = float((got.detach().double().cpu() - want.detach()).abs().max() / want.detach().abs().max())
        assert err < 2e-5, (what, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,stride", DW_BWD_EDGES)
def test_dwconv_backward_at_the_forward_edges(name, k, stride, hip_lib):
    """W < 4, H < k, planes of 255 / 256 / 257 items and rows on every dword alignment: the clamped addresses, the bit masks and
    the ragged 4-wide tail of the two backward kernels (the forward runs these shapes in tests/test_dwconv_staged.py)."""
    _dw_autograd_against_float64(dw_geometries(stride)[name] + (k, stride))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [DW_BWD_CAP, DW_BWD_PAD_BR], ids=["chunk-cap", "pad-bottom-right-only"])
def test_dwconv_backward_chunk_cap_and_one_sided_pad(shape, hip_lib):
    """520 x 520 outputs are 67 chunks of 4096: the weight-gradient grid stops at 64 and every workgroup walks its items with the
    grid stride.  Stride 2 on even H and W with k = 3 pads one row and column, all of it at the bottom / right."""
    _dw_autograd_against_float64(shape)
