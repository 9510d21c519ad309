"""CPU: the stereo matcher's specification (the comment above OccdStereoArgs in include/occdepth_amd.h) restated in
numpy, vectorised over rows -- the reference tests/test_stereo_gpu.py compares the kernels with, bit for bit -- and
its own checks: against a brute-force loop of the recurrence, the bound of S, the mirror symmetry, known-truth scenes
(the matcher must be a matcher, not just self-consistent), and the host logic around it (loader stub, PNG
quantisation, argument errors, f B of the synthetic calibration)."""
import ctypes
import struct
import types
import zlib

import numpy as np
import pytest
import torch

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
ABSENT = 1 << 20
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


# ------------------------------------------------------------------------------------------------- the restatement
def gray_from_u8(rgb):
    """(..., 3, H, W) uint8 -> (..., H, W) uint8."""
    u = np.asarray(rgb).astype(np.int32)
    return ((77 * u[..., 0, :, :] + 150 * u[..., 1, :, :] + 29 * u[..., 2, :, :] + 128) >> 8).astype(np.uint8)


def gray_from_normalized_ref(img, mean=MEAN, std=STD):
    """(..., 3, H, W) float32 normalised -> uint8 gray; float32 arithmetic, every operation rounded once."""
    x = np.asarray(img, dtype=np.float32)
    m = np.asarray(mean, dtype=np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float32).reshape(3, 1, 1)
    v = (x * s + m) * np.float32(255.0)
    u = np.clip(np.rint(np.where(np.isnan(v), np.float32(0), v)), 0, 255).astype(np.uint8)
    return gray_from_u8(u)


def census_ref(g):
    """(H, W) uint8 -> (H, W) uint64: window 9 x 7, replicate borders, neighbours row-major from the top-left without the
    centre, bit k = neighbour k < centre."""
    H, W = g.shape
    pad = np.pad(g, ((3, 3), (4, 4)), mode="edge")
    word = np.zeros((H, W), dtype=np.uint64)
    k = 0
    for dy in range(7):
        for dx in range(9):
            if dy == 3 and dx == 4:
                continue
            word |= (pad[dy:dy + H, dx:dx + W] < g).astype(np.uint64) << np.uint64(k)
            k += 1
    assert k == 62
    return word


def popcount64(a):
    return _POP8[np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))].sum(-1).astype(np.int32)


def cost_volume(cl, cr, D, s):
    """C (H, W, D) int32: popcount(cl[y, x] ^ cr[y, x - s d]) inside the image, 62 outside."""
    H, W = cl.shape
    C = np.full((H, W, D), 62, dtype=np.int32)
    x = np.arange(W)
    for d in range(D):
        xr = x - s * d
        ok = (xr >= 0) & (xr < W)
        if ok.any():
            C[:, ok, d] = popcount64(cl[:, ok] ^ cr[:, xr[ok]])
    return C


def scan(C, p1, p2):
    """The recurrence along axis 0 of C (N, M, D), all M lines at once."""
    L = np.empty_like(C)
    L[0] = C[0]
    pad = np.full(C.shape[1:2] + (1,), ABSENT, dtype=C.dtype)
    for i in range(1, C.shape[0]):
        q = L[i - 1]
        m = q.min(-1, keepdims=True)
        lo = np.concatenate([pad, q[:, :-1]], -1) + p1
        hi = np.concatenate([q[:, 1:], pad], -1) + p1
        L[i] = C[i] + np.minimum(np.minimum(q, m + p2), np.minimum(lo, hi)) - m
    return L


def path_volumes(C, p1, p2):
    """The four path volumes (H, W, D) in the order left-to-right, right-to-left, downwards, upwards."""
    Ct = C.transpose(1, 0, 2)
    return [scan(Ct, p1, p2).transpose(1, 0, 2), scan(Ct[::-1], p1, p2)[::-1].transpose(1, 0, 2),
            scan(C, p1, p2), scan(C[::-1], p1, p2)[::-1]]


def right_disparity(S, s):
    """dR (H, W): argmin_d S[y, x' + s d, d] over the d that stay inside the image, lowest d on ties."""
    H, W, D = S.shape
    T = np.full((H, W, D), ABSENT, dtype=np.int32)
    x = np.arange(W)
    for d in range(D):
        xl = x + s * d
        ok = (xl >= 0) & (xl < W)
        T[:, ok, d] = S[:, xl[ok], d]
    return T.argmin(-1).astype(np.int32)


def match(L, R, D=192, s=1, p1=10, p2=120, uniqueness=95):
    """gray L, R (H, W) uint8 -> dict(census (2, H, W) uint64, S (H, W, D) uint16, d0 int32, flags uint8, disp float32)."""
    cl, cr = census_ref(L), census_ref(R)
    C = cost_volume(cl, cr, D, s)
    S = sum(path_volumes(C, p1, p2)).astype(np.int32)
    H, W = L.shape
    d0 = S.argmin(-1).astype(np.int32)
    best = np.take_along_axis(S, d0[..., None], -1)[..., 0]
    d = np.arange(D)
    S2 = np.where(np.abs(d[None, None] - d0[..., None]) > 1, S, ABSENT).min(-1)
    unique = 100 * best <= uniqueness * S2
    dR = right_disparity(S, s)
    xr = np.arange(W)[None] - s * d0
    inside = (xr >= 0) & (xr < W)
    consistent = inside & (np.abs(np.take_along_axis(dR, np.clip(xr, 0, W - 1), 1) - d0) <= 1)
    inner = (d0 >= 1) & (d0 <= D - 2)
    a = np.take_along_axis(S, np.clip(d0 - 1, 0, D - 1)[..., None], -1)[..., 0]
    b = np.take_along_axis(S, np.clip(d0 + 1, 0, D - 1)[..., None], -1)[..., 0]
    den = 2 * (a + b - 2 * best)
    ok = inner & (den > 0)
    sub = np.where(ok, (a - b).astype(np.float32) / np.where(ok, den, 1).astype(np.float32), np.float32(0))
    flags = (unique * 1 + consistent * 2 + inner * 4).astype(np.uint8)
    disp = np.where(flags == 7, d0.astype(np.float32) + sub.astype(np.float32), np.float32(0)).astype(np.float32)
    return {"census": np.stack([cl, cr]), "S": S.astype(np.uint16), "d0": d0, "flags": flags, "disp": disp}


def focal_baseline_ref(cam_k, cam_E):
    """float32(k[0][0][0] |t_0 - t_1|) in float64; cam_k (V, 3, 3), cam_E (V, 4, 4)."""
    k, E = np.asarray(cam_k, np.float64), np.asarray(cam_E, np.float64)
    t = E[0, :3, 3] - E[1, :3, 3]
    return np.float32(k[0, 0, 0] * np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))


def depth_ref(disp, fB):
    with np.errstate(divide="ignore"):
        return np.where(disp > 0, np.float32(fB) / disp, np.float32(0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ known-truth scenes
def _smooth(a, sigma=0.7, radius=3):
    t = np.arange(-radius, radius + 1)
    k = np.exp(-0.5 * (t / sigma) ** 2)
    k /= k.sum()
    p = np.pad(a, radius, mode="reflect")
    p = sum(k[i] * p[i:i + a.shape[0], :] for i in range(2 * radius + 1))
    return sum(k[i] * p[:, i:i + a.shape[1]] for i in range(2 * radius + 1))


def scene(H, W, D, seed):
    """-> L, R (H, W) uint8, truth (H, W) int32 disparity of the left image, visible (H, W) bool.  Smoothed noise; the
    background has disparity 6 in the upper half and grows by one every two rows below; a box in front has 28.  R is L
    warped forward to x - d, the larger disparity winning; holes are uniform random bytes."""
    rs = np.random.RandomState(seed)
    tex = _smooth(rs.rand(H, W + D))
    tex = (tex - tex.min()) / (tex.max() - tex.min()) * 255.0
    L = np.rint(tex[:, :W]).astype(np.uint8)
    y = np.arange(H)[:, None]
    truth = np.where(y < H // 2, 6, 6 + (y - H // 2) // 2) + np.zeros((1, W), dtype=np.int64)
    truth[H // 6:H // 2 + 4, W // 3:W // 3 + W // 4] = 28
    truth = truth.astype(np.int32)
    R = rs.randint(0, 256, (H, W)).astype(np.uint8)
    owner = np.full((H, W), -1, dtype=np.int32)                 # disparity of the left pixel a right pixel shows
    src = np.full((H, W), -1, dtype=np.int32)
    for x in range(W):
        xt = x - truth[:, x]
        rows = np.nonzero((xt >= 0) & (xt < W))[0]
        rows = rows[truth[rows, x] > owner[rows, xt[rows]]]
        owner[rows, xt[rows]] = truth[rows, x]
        src[rows, xt[rows]] = x
        R[rows, xt[rows]] = L[rows, x]
    visible = np.zeros((H, W), dtype=bool)
    ys, xts = np.nonzero(src >= 0)
    visible[ys, src[ys, xts]] = True
    return L, R, truth, visible


def normalized_from_u8(rgb, mean=MEAN, std=STD):
    """What the loader's ToTensor + Normalize give: float32 (u / 255 - mean) / std."""
    x = torch.from_numpy(np.asarray(rgb)).to(torch.float32) / 255.0
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    return (x - m) / s


def scene_quality(out, truth, visible):
    valid = out["flags"] == 7
    seen = (valid & visible).sum() / visible.sum()
    wrong = (np.abs(out["disp"] - truth)[valid] > 1).sum() / max(int(valid.sum()), 1)
    return float(seen), float(wrong)


SCENES = [(48, 160, 64), (37, 122, 64), (40, 200, 128)]
_cache = {}


def matched_scene(H, W, D, seed, s=1):
    """match() of a scene, computed once per process (the GPU tests share it)."""
    key = (H, W, D, seed, s)
    if key not in _cache:
        L, R, truth, visible = scene(H, W, D, seed)
        if s < 0:
            L, R, truth, visible = (np.ascontiguousarray(a[:, ::-1]) for a in (L, R, truth, visible))
        _cache[key] = (L, R, truth, visible, match(L, R, D, s))
    return _cache[key]


# ------------------------------------------------------------------------------------------------------------ tests
def test_census_bits_on_a_hand_case():
    g = np.full((7, 9), 10, dtype=np.uint8)
    g[0, 0] = 3            # neighbour 0 of the centre pixel (3, 4)
    g[3, 5] = 4            # the first neighbour after the centre: index 3 * 9 + 4 = 31
    g[6, 8] = 200          # brighter: no bit
    w = census_ref(g)
    assert int(w[3, 4]) == (1 << 0) | (1 << 31)
    assert int(w[0, 0]) == 0 and int(census_ref(np.zeros((3, 3), np.uint8)).max()) == 0
    # replicate border: the corner's window sees g[0, 0] = 3 wherever it is clamped, never anything darker
    assert popcount64(np.array([w[3, 4]]))[0] == 2


def _brute_paths(C, p1, p2):
    H, W, D = C.shape
    S = np.zeros((H, W, D), dtype=np.int64)
    for (dx, dy) in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        L = np.zeros((H, W, D), dtype=np.int64)
        ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
        xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
        for y in ys:
            for x in xs:
                qx, qy = x - dx, y - dy
                if not (0 <= qx < W and 0 <= qy < H):
                    L[y, x] = C[y, x]
                    continue
                q = L[qy, qx]
                m = int(q.min())
                for d in range(D):
                    terms = [int(q[d]), m + p2]
                    if d > 0:
                        terms.append(int(q[d - 1]) + p1)
                    if d + 1 < D:
                        terms.append(int(q[d + 1]) + p1)
                    L[y, x, d] = int(C[y, x, d]) + min(terms) - m
        S += L
    return S


@pytest.mark.parametrize("s", [1, -1])
def test_restatement_matches_brute_force_recurrence(s):
    rs = np.random.RandomState(5)
    L = rs.randint(0, 256, (9, 14)).astype(np.uint8)
    R = np.roll(L, -3 * s, axis=1)
    C = cost_volume(census_ref(L), census_ref(R), 64, s)
    # the cost, element by element
    cl, cr = census_ref(L), census_ref(R)
    for y, x, d in ((0, 0, 0), (4, 13, 5), (8, 2, 2), (3, 7, 63), (5, 0, 1)):
        xr = x - s * d
        want = bin(int(cl[y, x]) ^ int(cr[y, xr])).count("1") if 0 <= xr < 14 else 62
        assert C[y, x, d] == want
    S = sum(path_volumes(C, 10, 120))
    assert np.array_equal(S, _brute_paths(C, 10, 120))
    out = match(L, R, 64, s)
    assert np.array_equal(out["S"], S)


@pytest.mark.parametrize("p2", [120, 193])
def test_path_sum_bound(p2):
    """A path value stays within 0 .. 62 + P2 (a byte up to P2 = 193), so S <= 4 (62 + P2) fits uint16."""
    L, R, _, _ = scene(19, 61, 64, 1)
    vols = path_volumes(cost_volume(census_ref(L), census_ref(R), 64, 1), 10, p2)
    assert min(int(v.min()) for v in vols) >= 0 and max(int(v.max()) for v in vols) <= 62 + p2 <= 255
    S = matched_scene(37, 122, 64, 0)[4]["S"] if p2 == 120 else match(L, R, 64, 1, p2=p2)["S"]
    assert int(S.max()) <= 4 * (62 + p2)


@pytest.mark.parametrize("shape", [(37, 122, 64), (24, 90, 128)])
def test_mirror_property(shape):
    """Mirroring both images and matching with s = -1 gives exactly the mirrored result, on every pixel."""
    H, W, D = shape
    L, R, _, _ = scene(H, W, D, 1)
    a = match(L, R, D, 1)
    b = match(np.ascontiguousarray(L[:, ::-1]), np.ascontiguousarray(R[:, ::-1]), D, -1)
    assert np.array_equal(b["S"], a["S"][:, ::-1])
    for key in ("d0", "flags", "disp"):
        assert np.array_equal(b[key], a[key][:, ::-1]), key
    assert (a["flags"] == 7).mean() > 0.5


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", SCENES)
def test_known_truth_scenes(shape, seed):
    H, W, D = shape
    _, _, truth, visible, out = matched_scene(H, W, D, seed)
    seen, wrong = scene_quality(out, truth, visible)
    msg = "scene %s seed %d: valid among visible %.4f (>= 0.95), wrong among valid %.4f (<= 0.04)" % (shape, seed, seen, wrong)
    print(msg)
    assert seen >= 0.95 and wrong <= 0.04, msg


def test_gray_from_normalized_is_the_integer_formula():
    rs = np.random.RandomState(3)
    rgb = rs.randint(0, 256, (2, 3, 16, 40)).astype(np.uint8)
    rgb[0, :, 0, :6] = np.array([[0, 255, 0, 255, 1, 254]] * 3, dtype=np.uint8)
    assert np.array_equal(gray_from_normalized_ref(normalized_from_u8(rgb).numpy()), gray_from_u8(rgb))
    assert gray_from_u8(np.full((3, 1, 1), 255, np.uint8))[0, 0] == 255 and gray_from_u8(np.zeros((3, 1, 1), np.uint8))[0, 0] == 0


# ------------------------------------------------------------------------------------------------------- host logic
def test_load_depth_stub_through_a_fake_dataset_module_with_undo():
    from occdepth_amd import targets
    real = lambda path: np.ones((370, 1220), np.float32)
    mod = types.SimpleNamespace(load_depth=real, vox2pix=lambda: None)
    hook = targets.defer_dataset_stereo_depth(mod)
    assert hook.active and mod.load_depth is not real
    d = mod.load_depth("no/such/file.png")
    assert d.shape == (0, 0) and d.dtype == np.float32
    # what the dataset and the collate do with it: crop, flip, stack
    d = np.ascontiguousarray(np.fliplr(d[:370, :1220]))
    stacked = torch.stack([torch.from_numpy(d[None].copy()), torch.from_numpy(d[None].copy())])
    assert stacked.numel() == 0
    from occdepth_amd.models.OccDepth import OccDepth
    assert OccDepth._tables_absent({"gt_depth": stacked}, "gt_depth")
    assert targets.defer_dataset_stereo_depth(mod).saved == {}          # already stubbed: nothing more to save
    hook.undo()
    assert mod.load_depth is real and not hook.active
    hook.undo()                                                          # idempotent
    with targets.defer_dataset_stereo_depth(mod):
        assert mod.load_depth is not real
    assert mod.load_depth is real
    assert not targets.defer_dataset_stereo_depth(types.SimpleNamespace()).active     # nothing to rebind


def _decode_png16(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, {}
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks[tag] = chunks.get(tag, b"") + data
        pos += 12 + n
    W, H, depth, colour = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, colour) == (16, 0)
    rows = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), np.uint8).reshape(H, 1 + 2 * W)
    assert not rows[:, 0].any()
    return rows[:, 1:].copy().view(">u2").astype(np.uint16)


def test_depth_png_quantisation(tmp_path):
    from occdepth_amd import stereo
    depth = np.array([[0.0, 2.0, 1.0 / 512, 3.0 / 512, 255.99, 256.0, 300.0],
                      [np.nan, np.inf, -1.0, 10.123, 80.0, 0.001, 5.0 / 512]], dtype=np.float32)
    q = stereo.depth_to_png16(depth)
    assert q.dtype == np.uint16
    assert q.tolist() == [[0, 512, 0, 2, 65533, 65535, 65535], [0, 0, 0, 2591, 20480, 0, 2]]     # rint: halves go to even
    path = stereo.write_png16(str(tmp_path / "d.png"), q)
    assert np.array_equal(_decode_png16(path), q)
    back = _decode_png16(path).astype(np.float32) / 256.0           # load_depth
    ok = (depth > 0) & np.isfinite(depth) & (depth < 255.9)
    assert np.abs(back - depth)[ok].max() <= 0.5 / 256 + 1e-6
    with pytest.raises(ValueError):
        stereo.write_png16(str(tmp_path / "e.png"), q.astype(np.int32))


def test_wrappers_reject_cpu_tensors_and_bad_arguments():
    from occdepth_amd import hip, stereo
    gray = torch.zeros(1, 2, 8, 16, dtype=torch.uint8)
    for call in (lambda: stereo.census(gray), lambda: stereo.sgm_disparity(gray, 64),
                 lambda: stereo.gray_from_normalized(torch.zeros(1, 2, 3, 8, 16)),
                 lambda: stereo.stereo_depth(gray, None, None),
                 lambda: hip.stereo_sgm(torch.zeros(1, 2, 8, 16, dtype=torch.int64), 64),
                 lambda: hip.stereo_depth(torch.zeros(1, 8, 16), None, None)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    with pytest.raises(TypeError):
        stereo.census(np.zeros((1, 2, 8, 16), np.uint8))


def test_entry_points_validate_arguments_without_a_launch(hip_lib):
    from occdepth_amd import hip
    assert hip_lib.occd_stereo_census(None, None) == -1 and hip_lib.occd_stereo_sgm(None, None) == -1
    assert hip_lib.occd_stereo_depth(None, None) == -1
    assert hip_lib.occd_stereo_workspace_bytes(1, 37, 122, 64) == (37 * 122 * 4 * 64 + 255) // 256 * 256 + (37 * 122 + 255) // 256 * 256
    for bad in ((0, 8, 8, 64), (1, 0, 8, 64), (1, 8, -1, 64), (1, 8, 8, 0), (1, 8, 8, 96), (1, 8, 8, 320), (1, 8, 8, 32)):
        assert hip_lib.occd_stereo_workspace_bytes(*bad) == -1, bad
    buf = (ctypes.c_double * 64)()
    ptr = ctypes.addressof(buf)                           # never dereferenced: every call below is rejected

    def args(**kw):
        a = hip.StereoArgs()
        a.gray = a.census = a.workspace = a.S = a.d0 = a.flags = a.disp = a.depth = a.cam_k = a.cam_E = ptr
        a.batch, a.H, a.W, a.max_disp, a.p1, a.p2, a.uniqueness, a.calib_views = 1, 8, 16, 64, 10, 120, 95, 2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    sgm = lambda **kw: hip_lib.occd_stereo_sgm(ctypes.byref(args(**kw)), None)
    for kw in (dict(census=None), dict(workspace=None), dict(S=None), dict(d0=None), dict(flags=None), dict(disp=None),
               dict(batch=0), dict(H=0), dict(W=-3), dict(max_disp=0), dict(max_disp=100), dict(max_disp=320),
               dict(p1=121), dict(p1=-1), dict(p2=194, p1=10), dict(uniqueness=0), dict(uniqueness=101),
               dict(ida=ptr, ida_views=0)):
        assert sgm(**kw) == -1, kw
    for kw in (dict(gray=None), dict(census=None), dict(batch=0), dict(H=-1), dict(W=0)):
        assert hip_lib.occd_stereo_census(ctypes.byref(args(**kw)), None) == -1, kw
    for kw in (dict(disp=None), dict(depth=None), dict(cam_k=None), dict(cam_E=None), dict(calib_views=1), dict(W=0)):
        assert hip_lib.occd_stereo_depth(ctypes.byref(args(**kw)), None) == -1, kw


def test_baseline_and_fb_of_the_synthetic_calibration():
    from occdepth_amd import stereo, synthetic
    frame = synthetic.kitti_frame(batch=1, img_hw=(8, 16))
    k = frame["cam_k"][0].numpy()
    E64 = frame["T_velo_2_cam_f64"][0].numpy()
    t = E64[0, :3, 3] - E64[1, :3, 3]
    assert float(np.sqrt((t * t).sum())) == 0.54 == synthetic.STEREO_BASELINE_M
    fB = stereo.focal_baseline(k, E64)
    assert fB.dtype == np.float32 and fB == np.float32(707.0912 * 0.54) == focal_baseline_ref(k, E64)
    assert abs(float(fB) - 381.83) < 0.01
    # the batch's float32 extrinsics carry 0.54 rounded to float32: fB moves by less than 2 ulp
    fB32 = stereo.focal_baseline(k, frame["T_velo_2_cam"][0].numpy())
    assert abs(float(fB32) - float(fB)) <= 2 * float(np.spacing(fB))
    d = depth_ref(np.array([0.0, 1.0, 190.9], np.float32), fB)
    assert d[0] == 0 and d[1] == fB and 1.99 < d[2] < 2.01
