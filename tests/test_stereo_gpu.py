"""GPU: the stereo matcher's kernels (csrc/stereo.hip) against the numpy restatement of tests/test_stereo.py -- census
words, summed path costs, winners, flag bits and the float32 disparity bit for bit -- and the model-level wiring:
`OccDepth.step` builds the depth target from the batch's image pair when the switch is on, eagerly and inside the
captured training step."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from test_stereo import (MEAN, STD, depth_ref, focal_baseline_ref, gray_from_u8, match, matched_scene, normalized_from_u8,
                         scene)

pytestmark = pytest.mark.gpu

# H, W, D, frames (s per frame): the smallest shapes at which each path of the kernels can go wrong
CASES = {
    "19x61_D64": (19, 61, 64, (1,)),             # D > W: most candidates leave the image; odd sizes, partial census tiles
    "37x122_D64": (37, 122, 64, (1,)),           # one disparity per lane
    "40x200_D128": (40, 200, 128, (1,)),         # two per lane
    "24x250_D192": (24, 250, 192, (1,)),         # three per lane, the KITTI setting
    "37x122_D64_B2": (37, 122, 64, (1, -1)),     # frame 0 as it is, frame 1 mirrored, in one launch
}


def _case(name):
    H, W, D, dirs = CASES[name]
    frames = [matched_scene(H, W, D, seed, s) for seed, s in enumerate(dirs)]
    gray = torch.from_numpy(np.stack([np.stack([f[0], f[1]]) for f in frames]))
    return gray, D, dirs, [f[4] for f in frames]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_restatement_bit_for_bit(name, hip_lib):
    from occdepth_amd import stereo
    gray, D, dirs, want = _case(name)
    g = gray.cuda()
    flipped = torch.tensor([s < 0 for s in dirs]).cuda() if len(dirs) > 1 else None
    words = stereo.census(g).cpu().numpy().view(np.uint64)
    disp, (S, d0, flags) = stereo.sgm_disparity(g, D, flipped=flipped, return_aux=True)
    assert disp.dtype == torch.float32 and tuple(disp.shape) == (len(dirs),) + tuple(gray.shape[2:])
    S, d0, flags, disp = S.cpu().numpy().view(np.uint16), d0.cpu().numpy(), flags.cpu().numpy(), disp.cpu().numpy()
    for b, ref in enumerate(want):
        assert np.array_equal(words[b], ref["census"]), "census words, frame %d" % b
        assert np.array_equal(S[b], ref["S"]), "S, frame %d: %d of %d differ" % (b, (S[b] != ref["S"]).sum(), S[b].size)
        assert np.array_equal(d0[b], ref["d0"]), "d0, frame %d" % b
        assert np.array_equal(flags[b], ref["flags"]), "flags, frame %d" % b
        assert np.array_equal(_bits(disp[b]), _bits(ref["disp"])), "disparity bits, frame %d" % b
        assert (ref["flags"] == 7).mean() > 0.3                     # the comparison is not one of empty maps


def test_other_penalties_and_uniqueness(hip_lib):
    """P2 at its largest (a path value of 255 still fits its byte) and a strict uniqueness ratio."""
    from occdepth_amd import stereo
    L, R, _, _ = scene(19, 61, 64, 2)
    ref = match(L, R, 64, 1, p1=7, p2=193, uniqueness=60)
    g = torch.from_numpy(np.stack([L, R]))[None].cuda()
    disp, (S, d0, flags) = stereo.sgm_disparity(g, 64, p1=7, p2=193, uniqueness=60, return_aux=True)
    assert np.array_equal(S[0].cpu().numpy().view(np.uint16), ref["S"]) and int(ref["S"].max()) > 4 * 182
    assert np.array_equal(flags[0].cpu().numpy(), ref["flags"]) and np.array_equal(d0[0].cpu().numpy(), ref["d0"])
    assert np.array_equal(_bits(disp[0].cpu().numpy()), _bits(ref["disp"]))


def test_gray_from_a_normalised_image_is_the_integer_formula(hip_lib):
    from occdepth_amd import stereo
    rs = np.random.RandomState(3)
    rgb = rs.randint(0, 256, (2, 2, 3, 19, 61)).astype(np.uint8)
    rgb[0, 0, :, 0, :6] = np.array([[0, 255, 0, 255, 1, 254]] * 3, dtype=np.uint8)
    img = normalized_from_u8(rgb.reshape(4, 3, 19, 61)).reshape(2, 2, 3, 19, 61).cuda()
    got = stereo.gray_from_normalized(img, MEAN, STD)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), gray_from_u8(rgb))


def _calibration(B):
    from occdepth_amd import synthetic
    frame = synthetic.kitti_frame(batch=B, img_hw=(8, 16))
    return torch.stack(frame["cam_k"]).cuda(), torch.stack(frame["T_velo_2_cam_f64"]).cuda()


def test_depth_is_fb_over_disparity(hip_lib):
    """depth equal to float32(fB) / disp, or within 1 ulp of it: the only freedom is the cast of fB."""
    from occdepth_amd import stereo
    gray, D, dirs, want = _case("37x122_D64_B2")
    k, E = _calibration(2)
    ida = torch.eye(4).repeat(2, 2, 1, 1)
    ida[1, :, 0, 0] = -1.0
    depth = stereo.stereo_depth(gray.cuda(), k, E, ida=ida.cuda(), max_disp=D)
    assert tuple(depth.shape) == (2, 1, 37, 122) and depth.dtype == torch.float32
    fB = focal_baseline_ref(k[0].cpu().numpy(), E[0].cpu().numpy())
    for b, ref in enumerate(want):
        exp = depth_ref(ref["disp"], fB)
        got = depth[b, 0].cpu().numpy()
        assert np.array_equal(got == 0, ref["disp"] == 0)
        ulps = np.abs(_bits(got).astype(np.int64) - _bits(exp).astype(np.int64))
        print("frame %d: fB = %r, depth %s" % (b, fB, "bit-equal" if ulps.max() == 0 else "within %d ulp" % ulps.max()))
        assert ulps.max() <= 1
    # from a normalised float image: the same map
    rgb = np.repeat(gray.numpy()[:, :, None], 3, axis=2)                       # gray of (u, u, u) is u
    img = normalized_from_u8(rgb.reshape(4, 3, 37, 122)).reshape(2, 2, 3, 37, 122).cuda()
    assert torch.equal(stereo.stereo_depth(img, k, E, ida=ida.cuda(), max_disp=D), depth)


def test_invalid_arguments_launch_nothing(hip_lib):
    from occdepth_amd import hip, stereo
    H, W, D = 19, 61, 64
    words = torch.zeros(1, 2, H, W, dtype=torch.int64, device="cuda")
    need = hip_lib.occd_stereo_workspace_bytes(1, H, W, D)
    bufs = {"workspace": torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda"),
            "S": torch.full((1, H, W, D), 0x5A5A, dtype=torch.int16, device="cuda"),
            "d0": torch.full((1, H, W), -7, dtype=torch.int32, device="cuda"),
            "flags": torch.full((1, H, W), 0x5A, dtype=torch.uint8, device="cuda"),
            "disp": torch.full((1, H, W), -7.0, device="cuda")}
    before = {k: v.clone() for k, v in bufs.items()}

    def call(**kw):
        a = hip.StereoArgs()
        a.census = words.data_ptr()
        for k, v in bufs.items():
            setattr(a, k, v.data_ptr())
        a.batch, a.H, a.W, a.max_disp, a.p1, a.p2, a.uniqueness = 1, H, W, D, 10, 120, 95
        for k, v in kw.items():
            setattr(a, k, v)
        return hip_lib.occd_stereo_sgm(ctypes.byref(a), hip._stream())

    for kw in (dict(max_disp=96), dict(max_disp=32), dict(max_disp=320), dict(p1=121), dict(p2=194), dict(uniqueness=0),
               dict(uniqueness=101), dict(H=0), dict(W=-1), dict(batch=0), dict(S=None), dict(census=None)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], bufs[k]) for k in bufs)
    g = torch.zeros(1, 2, H, W, dtype=torch.uint8, device="cuda")
    for kw in (dict(max_disp=100), dict(p1=200), dict(p2=194), dict(uniqueness=0)):
        with pytest.raises(ValueError):
            stereo.sgm_disparity(g, **kw)
    assert call() == 0                                                         # and the valid call does run
    torch.cuda.synchronize()
    assert not torch.equal(before["S"], bufs["S"])


# ----------------------------------------------------------------------------------------------------- model level
SMALL_HW, SMALL_D = (96, 320), 64


def _scene_batch(batch, seed, flip=False):
    """kitti_small's batch with a known-truth scene as its (normalised) image pair and no `gt_depth`."""
    H, W = SMALL_HW
    L, R, _, _ = scene(H, W, SMALL_D, seed)
    pair = np.stack([L, R])
    if flip:
        pair = np.ascontiguousarray(pair[:, :, ::-1])
    rgb = np.repeat(pair[:, None], 3, axis=1)                                  # (2, 3, H, W); gray of (u, u, u) is u
    out = {k: v for k, v in batch.items() if k != "gt_depth"}
    out["img"] = normalized_from_u8(rgb)[None].to(batch["img"].device)
    if flip:
        ida = [m.clone() for m in batch["ida_mats"]]
        for m in ida:
            m[:, 0, 0] = -1.0
        out["ida_mats"] = ida
    return out, torch.from_numpy(pair)


@pytest.fixture(scope="module")
def small(hip_lib):
    from test_train_step import _small_train_setup
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m, batch = _small_train_setup("kitti_small", "cuda")
    assert tuple(batch["img"].shape[-2:]) == SMALL_HW and m.use_stereo_depth_gt and m.gpu_stereo is None
    return m.eval(), batch


def test_switch_off_drops_the_depth_loss(small):
    m0, batch = small
    m = copy.deepcopy(m0)
    b, _ = _scene_batch(batch, 0)
    m.step(b, "train", None)
    assert "train/loss_depth" not in m.logged and "train/loss" in m.logged


def test_step_builds_the_depth_target_from_the_image_pair(small):
    from occdepth_amd import stereo
    m0, batch = small
    m = copy.deepcopy(m0).enable_stereo_depth(max_disp=SMALL_D)
    b, pair = _scene_batch(batch, 0)
    keys = sorted(b)
    seen = []
    real = m.depth_loss_fn.get_depth_loss
    m.depth_loss_fn.get_depth_loss = lambda gt, pred: (seen.append(gt.detach().clone()), real(gt, pred))[1]
    m.step(b, "train", None)
    assert sorted(b) == keys                                                   # the batch is not modified
    built = float(m.logged["train/loss_depth"])
    k = torch.stack(b["cam_k"]).cuda()
    E = torch.stack(b["T_velo_2_cam"]).cuda()
    gt = stereo.stereo_depth(b["img"], k, E, ida=torch.stack(b["ida_mats"]).cuda(), max_disp=SMALL_D)
    assert tuple(gt.shape) == (1, 1) + SMALL_HW
    m.step(dict(b, gt_depth=gt), "train", None)
    given = float(m.logged["train/loss_depth"])
    # the target itself: the same kernels on the same numbers, so the very same map -- and the restatement's
    assert len(seen) == 2 and torch.equal(seen[0], seen[1]) and torch.equal(seen[0], gt)
    ref = match(pair[0].numpy(), pair[1].numpy(), SMALL_D, 1)
    fB = focal_baseline_ref(k[0].cpu().numpy(), E[0].double().cpu().numpy())
    ulps = np.abs(_bits(gt[0, 0].cpu().numpy()).astype(np.int64) - _bits(depth_ref(ref["disp"], fB)).astype(np.int64))
    assert ulps.max() <= 1
    cells = m.depth_loss_fn._get_downsampled_gt_depth(gt)
    measured = int((cells.amax(1) > 0).sum())
    print("loss_depth built in the step %r, given as gt_depth %r; measured cells %d of %d" % (built, given, measured, cells.shape[0]))
    assert measured > 0 and np.isfinite(built) and built > 0
    # the loss runs the network a second time: the backend may pick another convolution algorithm on a later call, so
    # the two predictions are held to 1e-6 relative, not to the bit (the printed values show which it was)
    assert abs(built - given) <= 1e-6 * abs(given)
    # a "test" step builds nothing; a batch that brings gt_depth is used as it is (checked above: seen[1] is gt)
    m.step(b, "test", None)
    assert "test/loss_depth" not in m.logged and len(seen) == 2


def test_flipped_batch_gives_the_mirrored_map(small):
    m0, batch = small
    m = copy.deepcopy(m0).enable_stereo_depth(max_disp=SMALL_D)
    plain = m.stereo_depth_on_gpu(_scene_batch(batch, 1)[0])
    flipped = m.stereo_depth_on_gpu(_scene_batch(batch, 1, flip=True)[0])
    assert float((plain > 0).float().mean()) > 0.5
    assert torch.equal(flipped, plain.flip(-1))
    gray = _scene_batch(batch, 1)[1][None].cuda()                              # `img_gray_u8` is matched instead of `img`
    b = dict(_scene_batch(batch, 2)[0], img_gray_u8=gray)
    assert torch.equal(m.stereo_depth_on_gpu(b), plain)


def test_switch_on_says_what_is_missing(small):
    m0, batch = small
    m = copy.deepcopy(m0).enable_stereo_depth(max_disp=SMALL_D)
    b, _ = _scene_batch(batch, 0)
    with pytest.raises(ValueError, match="both views"):
        m.stereo_depth_on_gpu(dict(b, img=b["img"][:, :1]))
    for key in ("cam_k", "T_velo_2_cam"):
        with pytest.raises(KeyError, match=key):
            m.stereo_depth_on_gpu({k: v for k, v in b.items() if k != key})
    m.dataset = "NYU"
    with pytest.raises(NotImplementedError, match="NYU"):
        m.stereo_depth_on_gpu(b)
    m.dataset = "kitti"
    with pytest.raises(RuntimeError, match="GPU"):
        m.stereo_depth_on_gpu(dict(b, img=b["img"].cpu()))
    with pytest.raises(ValueError, match="max_disp"):
        m.enable_stereo_depth(max_disp=100)
    with pytest.raises(RuntimeError, match="enable_stereo_depth"):
        copy.deepcopy(m0).stereo_depth_on_gpu(b)


def test_captured_step_matches_the_image_pair_it_is_fed(small):
    """The fast training step captured on one image pair and replayed after another pair is copied in gives the eager
    step's loss_depth on that pair: the matcher runs inside the graph, on the static batch's current content."""
    m0, batch = small
    first, _ = _scene_batch(batch, 0)
    second, _ = _scene_batch(batch, 2)
    eager = copy.deepcopy(m0).train().enable_stereo_depth(max_disp=SMALL_D)
    eager.step(second, "train", None)
    want = float(eager.logged["train/loss_depth"])
    eager.step(first, "train", None)
    other = float(eager.logged["train/loss_depth"])
    m = copy.deepcopy(m0).train().enable_stereo_depth(max_disp=SMALL_D).enable_fast_train()
    m._opt = torch.optim.AdamW(m.parameters(), lr=0.0, weight_decay=0.0, fused=True)      # the parameters stay put
    m.training_step(first, 0)                                   # captures (the warm-up runs on a snapshot), replays
    st = m._fast_train
    assert st["graph"] is not None and st["graph"].graph is not None, getattr(st["graph"], "error", None)
    m.training_step(second, 1)                                  # copies the new pair in, replays
    got = float(m.logged["train/loss_depth"])
    print("loss_depth: replayed %r, eager %r (on the captured pair: %r)" % (got, want, other))
    assert abs(want - other) > 1e-3 * abs(want)                 # the two pairs do give different losses
    # the bound of test_whole_step_hipgraph_matches_eager_gpu's first step: the backend may choose other convolution
    # algorithms inside a capture; the depth target itself is the same integer pipeline
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
