"""Depthwise 2-D convolution, LDS tile staged in 16-byte chunks (dwconv2d_kernel<K, STRIDE, true>, csrc/nchw2d.hip;
index arithmetic in csrc/dwconv_stage.h) against the element-wise staging it replaced, which stays selectable through
occd_dwconv2d_set_stage(0).

GPU: both forms in one process -- y and the pooling partials must be the same bits -- and both against the float64 emulation.
CPU: the kernel's loads are unconditional and masked, so no output shows a read outside a plane; tests/dwconv_stage_walk.cpp
replays every (workgroup, thread, pass) through the header's own functions and checks the addresses and the tile."""
import os
import shutil
import subprocess

import pytest
import torch

import emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block_edge(n, stride):
    """(H, W) whose item count Ho * ceil(Wo / 4) is n in {255, 256, 257}: the 256-item block boundary of the partials."""
    Ho, Wo = {255: (15, 66), 256: (16, 61), 257: (257, 4)}[n]          # 15 x 17, 16 x 16, 257 x 1 items
    return (Ho * stride, Wo * stride if Wo > 4 else 4)                 # (W = 4, stride 2: Wo = 2, still one item per row)


def geometries(stride):
    """name -> (B, C, H, W): the smallest shapes at which chunked staging can go wrong."""
    g = {
        "w1": (1, 3, 5, 1), "w3": (1, 3, 6, 3),                        # W < 4: the scalar path
        "w4": (1, 3, 5, 4), "w5": (1, 3, 5, 5), "w7": (2, 2, 3, 7),    # clamped edge chunks left and right; H * W = 25, 21 with
        "w39": (1, 3, 3, 39),                                          # >= 3 planes: interior planes on every dword alignment
        "h1": (1, 3, 1, 9), "h2": (1, 3, 2, 9),                        # k = 5: most staged rows lie outside the image
        "items120": (1, 1, 12 * stride, 39 * stride),                  # one plane of 120 items for 256 threads (12 x 39 outputs)
    }
    for n in (255, 256, 257):
        g["items%d" % n] = (1, 1) + _block_edge(n, stride)
    return g


NAMES = list(geometries(1))
# occd_dwconv2d_set_stage: 0 element-wise staging (the form before), 2 chunks with one plane per workgroup everywhere, 1 the default
# (chunks; planes of at most 128 items two to a workgroup -- most of the shapes here)
FORMS = (0, 2, 1)


def test_geometries_are_what_they_claim():
    for stride in (1, 2):
        g = geometries(stride)
        for n in (120, 255, 256, 257):
            _, _, H, W = g["items%d" % n]
            Ho, Wo = -(-H // stride), -(-W // stride)
            assert Ho * ((Wo + 3) // 4) == n
        assert all(v[0] * v[1] >= 3 and (v[2] * v[3]) % 4 for v in (g["w5"], g["w7"], g["w39"]))
        assert max(v[0] * v[1] * v[2] * v[3] for v in g.values()) < 5000


def _inputs(shape, k):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 * H + 10 * W + k)
    x = torch.randn(B, C, H, W, generator=gen)
    w = torch.randn(C, 1, k, k, generator=gen) * 0.3
    return x, w, torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("name", NAMES)
def test_dwconv_chunked_staging_gpu(name, k, stride, hip_lib):
    from occdepth_amd import hip
    shape = geometries(stride)[name]
    B, C, H, W = shape
    x, w, sc, sh = _inputs(shape, k)
    y_ref, part_ref, plane = emu.dwconv2d_same_pool(x, w, sc, sh, stride, "swish")
    xd, wd, scd, shd = x.cuda(), w.cuda(), sc.cuda(), sh.cuda()
    # the same planes on a 128-byte pitch with NaN between them (the view of an expand GEMM's padded_rows result)
    xp = hip.padded_rows((B, C, H * W), "cuda")
    torch.as_strided(xp, (B, C, xp.stride(1)), (xp.stride(0), xp.stride(1), 1)).fill_(float("nan"))
    xp.copy_(xd.view(B, C, H * W))
    got = {}
    for form in FORMS:
        old = hip_lib.occd_dwconv2d_set_stage(form)
        try:
            got[form] = (hip.dwconv2d_same(xd, wd, scd, shd, stride, "swish"),                        # without pooling
                         hip.dwconv2d_same_pool(xd, wd, scd, shd, stride, "swish"),                   # with pooling
                         hip.dwconv2d_same_pool(xp.view(B, C, H, W), wd, scd, shd, stride, "swish"))  # ... on the padded pitch
        finally:
            hip_lib.occd_dwconv2d_set_stage(old)
    assert hip_lib.occd_dwconv2d_set_stage(1) == 1                     # the default is the chunked form
    nblk = hip_lib.occd_dwconv2d_pool_blocks(-(-H // stride), -(-W // stride))
    for form in FORMS:
        y0, (y1, p1, n1), (y2, p2, n2) = got[form]
        assert n1 == n2 == plane and p1.shape == p2.shape == (B * C, nblk)
        for y in (y0, y1, y2):
            assert torch.allclose(y.cpu(), y_ref, rtol=1e-5, atol=1e-5), (form, float((y.cpu() - y_ref).abs().max()))
        # a plane's partials sum `plane` outputs that each meet the bound above
        for p in (p1, p2):
            assert torch.allclose(p.double().sum(1).cpu(), part_ref.double().sum(1), rtol=1e-5, atol=1e-5 * plane)
    for form in FORMS[1:]:                                             # new forms against the old form: the same bits
        for a, b in zip(got[0], got[form]):
            if isinstance(a, tuple):
                assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), form
            else:
                assert torch.equal(a, b), form
        assert torch.equal(got[form][0], got[form][1][0]) and torch.equal(got[form][1][0], got[form][2][0])
        assert torch.equal(got[form][1][1], got[form][2][1])


# ---- CPU: the address arithmetic of the chunked staging
FRAME = [(185, 610, 3, 1), (185, 610, 3, 2), (93, 305, 3, 1), (93, 305, 5, 2), (47, 153, 5, 1), (47, 153, 3, 2), (24, 77, 3, 1),
         (24, 77, 5, 1), (24, 77, 5, 2), (12, 39, 5, 1), (12, 39, 3, 1)]    # the depthwise launches of a config-2 frame


def test_dwconv_chunk_addresses_cpu(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "no system C++ compiler"
    exe = str(tmp_path / "dwconv_stage_walk")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "occdepth_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dwconv_stage_walk.cpp"), "-o", exe])
    args = []
    for stride in (1, 2):
        for name, (B, C, H, W) in geometries(stride).items():
            if W < 4:
                continue                                               # (the element-wise form runs these)
            for k in (3, 5):
                for xps in (H * W, (H * W + 31) // 32 * 32):           # dense, and the 128-byte pitch of hip.padded_rows
                    args += [B * C, H, W, k, stride, xps]
    for H, W, k, stride in FRAME:                                      # two planes of each; the LAST plane ends the buffer
        args += [2, H, W, k, stride, H * W]
    r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") == len(args) // 6


def test_dwconv_stage_export_in_header():
    from occdepth_amd import abi
    import ctypes
    assert abi.EXPORTS["occd_dwconv2d_set_stage"] == (ctypes.c_int32, [ctypes.c_int32])
    assert abi.ABI_VERSION == 22
