"""GPU: occd_render_voxels against the numpy restatement of tests/test_render.py (`cast_ref` in float64, `colour_ref`), the
public module on top of it, the model hook and the command-line tool.  The shapes are the smallest at which each path can
still go wrong: odd image sizes (partial 8 x 8 tiles), several workgroups, three kinds of view and two frames in one launch."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from test_render import (KITTI_VOXEL, MAX_DISAGREE, cast_ref, colour_ref, decode_png, disagreement, kitti_calibration,
                         kitti_origin, make_scene, rays, scene_views, camera_cell)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: dims, camera (H, W), BEV pixels per voxel or None, oblique (H, W) or None, frames
CASES = {"24x20x12": ((24, 20, 12), (19, 61), None, None, 1),
         "64x64x16": ((64, 64, 16), (37, 122), 2, (91, 122), 2)}


def _views(dims, cam_hw, ppv, obl):
    v = scene_views(dims, cam_hw, ppv or 1, obl)
    if ppv is None:
        v.pop("bev")
    return v


@pytest.fixture(scope="module", params=sorted(CASES))
def scene(request, hip_lib):
    """Volumes, masks, views and the two restatements' results (computed once, never modified)."""
    dims, cam_hw, ppv, obl, B = CASES[request.param]
    vols = np.stack([make_scene(dims, seed=11 + b) for b in range(B)])
    rng = np.random.RandomState(1)
    fov = rng.rand(*vols.shape) < 0.7
    views = _views(dims, cam_hw, ppv, obl)
    ref64, ref32 = {}, {}
    for name, (view, (H, W)) in views.items():
        ref64[name] = [cast_ref(vols[b], *rays(view, H, W, np.float64), np.float64) for b in range(B)]
        ref32[name] = [cast_ref(vols[b], *rays(view, H, W, np.float32), np.float32) for b in range(B)]
    return {"dims": dims, "B": B, "vols": vols, "fov": fov, "views": views, "ref64": ref64, "ref32": ref32}


def _launch(scene, labels, **kw):
    from occdepth_amd import render
    names = list(scene["views"])
    views = [torch.from_numpy(scene["views"][n][0]) for n in names]
    sizes = [scene["views"][n][1] for n in names]
    return names, render.render_labels(labels, views, sizes, **kw)


def test_kernel_against_restatement(scene):
    from occdepth_amd import render
    pal = render.palette("kitti").numpy()
    labels = torch.from_numpy(scene["vols"]).to(DEV)
    names, (rgb, hit, face, depth) = _launch(scene, labels, fov=torch.from_numpy(scene["fov"]).to(DEV), palette="kitti",
                                             return_aux=True)
    for i, name in enumerate(names):
        H, W = scene["views"][name][1]
        assert tuple(rgb[i].shape) == (scene["B"], H, W, 3) and rgb[i].dtype == torch.uint8
        for b in range(scene["B"]):
            got = (hit[i][b].cpu().numpy(), face[i][b].cpu().numpy(), depth[i][b].cpu().numpy())
            r64, r32 = scene["ref64"][name][b], scene["ref32"][name][b]
            share, rel = disagreement(got, r64)
            own_share, own_rel = disagreement(r32, r64)
            print(f"{name} b{b} {W}x{H}: kernel disagree {share:.2e} depth rel {rel:.2e}; float32 restatement {own_share:.2e} {own_rel:.2e}")
            assert share <= MAX_DISAGREE, (name, b, share)
            assert rel <= 4 * max(own_rel, 1e-6), (name, b, rel, own_rel)
            miss = got[0] < 0
            assert np.isposinf(got[2][miss]).all() and (got[1][miss] == 3).all()
            agree = (got[0] == r64[0]) & (got[1] == r64[1])
            want = colour_ref(scene["vols"][b], r64[0], r64[1], pal, fov=scene["fov"][b])
            img = rgb[i][b].cpu().numpy()
            assert np.array_equal(img[agree], want[agree])                       # exact wherever (hit, face) agree
            assert (img[miss] == np.array(render.BACKGROUND, dtype=np.uint8)).all()
            # and exact everywhere given the kernel's own (hit, face): the colour rule has no float in it
            assert np.array_equal(img, colour_ref(scene["vols"][b], got[0], got[1], pal, fov=scene["fov"][b]))


def test_canvas_outside_a_view_is_background(scene):
    """Views of different sizes share one canvas: what lies outside a view's rectangle is background, hit -1."""
    from occdepth_amd import hip, render
    names = list(scene["views"])
    sizes = [scene["views"][n][1] for n in names]
    H, W = max(s[0] for s in sizes) + 3, max(s[1] for s in sizes) + 5
    views = torch.stack([torch.from_numpy(scene["views"][n][0]) for n in names])[None].expand(scene["B"], -1, -1).contiguous().to(DEV)
    labels = torch.from_numpy(scene["vols"]).to(DEV)
    rgb, hit, face, depth = hip.render_voxels(labels, views, (H, W), render.palette("kitti").to(DEV), view_sizes=sizes, aux=True)
    tight = _launch(scene, labels, return_aux=True)[1][1]                  # the hits on the smallest common canvas
    for i, (h, w) in enumerate(sizes):
        outside = torch.ones(H, W, dtype=torch.bool, device=DEV)
        outside[:h, :w] = False
        assert (hit[:, i][:, outside] == -1).all() and (rgb[:, i][:, outside] == 255).all()
        assert torch.equal(hit[:, i, :h, :w], tight[i])


def test_camera_inside_an_occupied_voxel_and_axis_parallel_rays(hip_lib):
    from occdepth_amd import render
    dims, (H, W) = (24, 20, 12), (19, 61)
    k, E = kitti_calibration(W)
    cam = render.camera_view(torch.from_numpy(k), torch.from_numpy(E), kitti_origin(dims), KITTI_VOXEL)
    full = torch.full((1,) + dims, 4, dtype=torch.uint8, device=DEV)
    rgb, hit, face, depth = render.render_labels(full, [cam, render.bev_view(dims, 1, device=DEV)], [(H, W), render.bev_size(dims, 1)],
                                                 return_aux=True, palette="kitti")
    c = camera_cell(dims)
    assert (hit[0] == (c[0] * dims[1] + c[1]) * dims[2] + c[2]).all() and (face[0] == 3).all() and (depth[0] == 0).all()
    assert (rgb[0] == render.palette("kitti")[4].to(DEV)).all()                   # face 3 is unshaded
    x, y = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), indexing="ij")
    top = ((x * dims[1] + y) * dims[2] + dims[2] - 1)[::-1, ::-1]
    assert np.array_equal(hit[1][0].cpu().numpy(), top) and (face[1] == 2).all() and (depth[1] == 1).all()
    empty = torch.zeros_like(full)                                                # every ray walks the whole grid and ends
    rgb, hit, face, depth = render.render_labels(empty, [cam, render.bev_view(dims, 1, device=DEV)], [(H, W), render.bev_size(dims, 1)],
                                                 return_aux=True)
    assert all((h == -1).all() for h in hit) and all((r == 255).all() for r in rgb) and all(torch.isposinf(d).all() for d in depth)


def test_degenerate_views_give_background(hip_lib):
    from occdepth_amd import render
    dims = (24, 20, 12)
    full = torch.full((1,) + dims, 4, dtype=torch.uint8, device=DEV)
    away = render.bev_view(dims, 1, device="cpu").clone()
    away[11] = 1.0                                                    # looks up, away from the volume below it
    far = torch.zeros(18)
    far[0:3] = torch.tensor([-1e30, 3.0, 3.0])                        # far outside, the x and z components of dir are zero
    far[10] = 1.0
    beside = torch.zeros(18)
    beside[0:3] = torch.tensor([5.0, 5.0, 40.0])                      # parallel to the volume, above it
    beside[9] = 1.0
    huge = torch.zeros(18)
    huge[0:3] = torch.tensor([3e38, 3e38, 3e38])                      # origin + (u + 1/2) ou overflows to inf
    huge[3:6] = 3e38
    huge[9:12] = 1.0
    for v in (away, far, beside, huge):
        rgb, hit, face, depth = render.render_labels(full, v, (20, 24), return_aux=True)
        assert (hit == -1).all() and (rgb == 255).all() and (face == 3).all() and torch.isposinf(depth).all()


def test_label_widths_and_logits(scene):
    from occdepth_amd import hip, render
    vols = torch.from_numpy(scene["vols"]).to(DEV)
    names, (rgb8, hit8, _, _) = _launch(scene, vols, return_aux=True, palette="kitti")
    for dtype in (np.int16, np.int32, np.uint16):
        wide = torch.from_numpy(scene["vols"].astype(dtype)).to(DEV)
        _, (rgb16, hit16, _, _) = _launch(scene, wide, return_aux=True, palette="kitti")
        assert all(torch.equal(a, b) for a, b in zip(rgb8, rgb16)) and all(torch.equal(a, b) for a, b in zip(hit8, hit16))
    # logits as the eval path returns them: a channels-last view of rows wider than C
    B, C = scene["B"], 20
    X, Y, Z = scene["dims"]
    rows = torch.randn(B, X, Y, Z, 24, device=DEV)
    logits = rows[..., :C].permute(0, 4, 1, 2, 3)
    assert not logits.is_contiguous()
    arg = logits.argmax(1)
    lab = hip.argmax_labels_u16(logits)
    assert lab.dtype == torch.int16 and torch.equal(lab.to(torch.int64), arg)
    _, a = _launch(scene, arg.to(torch.uint8))
    names = list(scene["views"])
    b = render.render_logits(logits, [torch.from_numpy(scene["views"][n][0]) for n in names], [scene["views"][n][1] for n in names])
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_error_mode_and_overlay(scene):
    from occdepth_amd import render
    pal = render.palette("kitti").numpy()
    rng = np.random.RandomState(2)
    pred = scene["vols"]
    targ = pred.copy()
    change = rng.rand(*pred.shape) < 0.3
    targ[change] = rng.randint(0, 20, size=int(change.sum()))
    targ[rng.rand(*pred.shape) < 0.05] = 255
    names = list(scene["views"])
    H, W = max(scene["views"][n][1][0] for n in names), max(scene["views"][n][1][1] for n in names)
    back = rng.randint(0, 256, size=(scene["B"], len(names), H, W, 3)).astype(np.uint8)
    fov_t = torch.from_numpy(scene["fov"]).to(DEV)
    for alpha in (0, 96, 256):
        _, (rgb, hit, face, depth) = _launch(scene, torch.from_numpy(pred).to(DEV), target=torch.from_numpy(targ).to(DEV),
                                             mode="error", fov=fov_t, palette="kitti", return_aux=True,
                                             background=torch.from_numpy(back).to(DEV), alpha=alpha)
        for i, name in enumerate(names):
            view, (h, w) = scene["views"][name]
            for b in range(scene["B"]):
                got = (hit[i][b].cpu().numpy(), face[i][b].cpu().numpy(), depth[i][b].cpu().numpy())
                if alpha == 96:
                    r64 = cast_ref(pred[b], *rays(view, h, w, np.float64), np.float64, target=targ[b])
                    assert disagreement(got, r64)[0] <= MAX_DISAGREE
                    vis = got[0][got[0] >= 0]
                    assert (targ[b].reshape(-1)[vis] != 255).all()                  # ignored voxels are transparent
                want = colour_ref(pred[b], got[0], got[1], pal, fov=scene["fov"][b], target=targ[b],
                                  background=back[b, i, :h, :w], alpha=alpha)
                assert np.array_equal(rgb[i][b].cpu().numpy(), want)
                if alpha == 0:
                    assert np.array_equal(want, back[b, i, :h, :w])


def test_render_is_capture_safe(hip_lib):
    from occdepth_amd import render, train_graph
    dims, size = (24, 20, 12), (19, 61)
    k, E = kitti_calibration(size[1])
    views = torch.stack([render.camera_view(torch.from_numpy(k), torch.from_numpy(E), kitti_origin(dims), KITTI_VOXEL),
                         render.oblique_view(dims, size, device="cpu")]).to(DEV)
    a, b = (torch.from_numpy(make_scene(dims, seed=s)[None]).to(DEV) for s in (21, 22))
    want_a, want_b = render.render_labels(a, views, size), render.render_labels(b, views, size)   # also warms the palette
    assert not torch.equal(want_a, want_b)
    static = a.clone()
    torch.cuda.synchronize()
    g = train_graph.new_graph()
    with torch.cuda.graph(g):
        out = render.render_labels(static, views, size)
    train_graph.seal_graph(g)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    static.copy_(b)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b)


# ------------------------------------------------------------------------------------------------- model hook and tool
@pytest.fixture(scope="module")
def model_run(hip_lib, tmp_path_factory):
    """The kitti_small model: forward and test_step with the hook off, then one test_step with it on."""
    from occdepth_amd import hip
    from test_vox2pix_gpu import _train_setup, _without
    m, full = _train_setup()
    m = m.eval()
    batch = _without(full)
    batch.pop("T_velo_2_cam_f64")
    B = len(batch["cam_k"])
    n = int(np.prod(m.full_scene_size))
    g = torch.Generator().manual_seed(5)
    batch["fov_mask_1"] = [(torch.rand(n, generator=g) < 0.6).to(DEV) for _ in range(B)]
    batch["sequence"] = ["08"] * B
    batch["frame_id"] = ["%06d" % (5 * i) for i in range(B)]
    out_dir = str(tmp_path_factory.mktemp("render"))
    with torch.no_grad():
        assert m.render is None
        m.test_step(batch, 0)                                       # warm: whatever a first step packs or caches
        m.test_metrics.reset()
        with hip.profile() as prof_off:
            logit_off = m(batch)["ssc_logit"].detach().clone()
            m.test_step(batch, 0)
        hist_off = m.test_metrics.hist.clone()
        m.test_metrics.reset()
        m.enable_render(out_dir, views=("camera", "bev"))
        with hip.profile() as prof_on:
            logit_on = m(batch)["ssc_logit"].detach().clone()
            m.test_step(batch, 0)
        hist_on = m.test_metrics.hist.clone()
    return {"m": m, "batch": batch, "B": B, "out_dir": out_dir, "logit_off": logit_off, "logit_on": logit_on,
            "rows_off": dict(prof_off.rows), "rows_on": dict(prof_on.rows), "hist_off": hist_off, "hist_on": hist_on}


def _expected_images(run):
    from occdepth_amd import render
    m, batch = run["m"], run["batch"]
    dims = tuple(int(d) for d in run["logit_on"].shape[2:])
    views, sizes = m._render_views(batch, dims, batch["img"].shape[-2:], torch.device(DEV), names=("camera", "bev"))
    fov = torch.stack(batch["fov_mask_1"]).reshape((run["B"],) + dims)
    return sizes, render.render_logits(run["logit_on"], views, sizes, fov=fov, palette="kitti")


def test_model_hook_end_to_end(model_run):
    run = model_run
    assert torch.equal(run["logit_off"], run["logit_on"]) and torch.equal(run["hist_off"], run["hist_on"])
    assert not any(k.startswith("render_voxels") for k in run["rows_off"])
    on = {k: v for k, v in run["rows_on"].items() if k.startswith("render_voxels")}
    assert len(on) == 1 and list(on.values())[0]["launches"] == 1                 # both views, all frames: one launch
    others = lambda rows: {k: v["launches"] for k, v in rows.items() if not k.startswith(("render_voxels", "argmax"))}
    assert others(run["rows_off"]) == others(run["rows_on"])                        # the step itself launches what it did
    sizes, images = _expected_images(run)
    assert sizes[0] == tuple(run["batch"]["img"].shape[-2:]) and sizes[1] == (512, 512)
    files = sorted(os.listdir(os.path.join(run["out_dir"], "08")))
    assert files == sorted("%06d_%s.png" % (5 * i, v) for i in range(run["B"]) for v in ("camera", "bev"))
    assert sorted(run["m"].render["paths"]) == sorted(os.path.join(run["out_dir"], "08", f) for f in files)
    for i in range(run["B"]):
        for j, v in enumerate(("camera", "bev")):
            img = decode_png(os.path.join(run["out_dir"], "08", "%06d_%s.png" % (5 * i, v)))
            assert np.array_equal(img, images[j][i].cpu().numpy())
            assert (img != 255).any()                                                # something was drawn
    # `every` and `max_frames`
    m = run["m"]
    m.enable_render(os.path.join(run["out_dir"], "second"), every=2, views=("oblique",), mode="error", overlay=True, max_frames=1)
    with torch.no_grad():
        m.test_step(run["batch"], 0)
        m.test_step(run["batch"], 1)                                                 # skipped
    assert m.render["seen"] == 2 and m.render["written"] == 1
    assert os.listdir(os.path.join(run["out_dir"], "second", "08")) == ["000000_oblique.png"]
    m.enable_render(os.path.join(run["out_dir"], "third"), views=("camera",), overlay=True)
    with torch.no_grad():
        m.test_step(run["batch"], 0)
    over = decode_png(os.path.join(run["out_dir"], "third", "08", "000000_camera.png"))
    assert over.shape == images[0][0].shape and not np.array_equal(over, images[0][0].cpu().numpy())
    m.render = None


def test_tool_renders_the_pickles_like_the_hook(model_run, tmp_path):
    from occdepth_amd import output
    run = model_run
    paths = output.write_outputs(run["logit_on"], run["batch"], str(tmp_path / "pred"), "kitti")
    assert len(paths) == run["B"]
    spec = importlib.util.spec_from_file_location("render_predictions", os.path.join(ROOT, "tools", "render_predictions.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    H, W = run["batch"]["img"].shape[-2:]
    written = tool.main([str(tmp_path / "pred"), "--out", str(tmp_path / "png"), "--image-size", str(int(H)), str(int(W)),
                         "--voxel-size", "0.2", "--batch", "8"])
    assert len(written) == 2 * run["B"]
    _, images = _expected_images(run)
    for i in range(run["B"]):
        for j, v in enumerate(("camera", "bev")):
            img = decode_png(str(tmp_path / "png" / "08" / ("%06d_%s.png" % (5 * i, v))))
            assert np.array_equal(img, images[j][i].cpu().numpy())
    if "target" not in run["batch"]:
        with pytest.raises(SystemExit):
            tool.main([str(tmp_path / "pred"), "--target"])
        return
    from occdepth_amd import hip, render
    tool.main([str(tmp_path / "pred"), "--out", str(tmp_path / "err"), "--views", "bev", "--target", "--batch", "1"])
    dims = tuple(int(d) for d in run["logit_on"].shape[2:])
    target = torch.stack([torch.as_tensor(t) for t in run["batch"]["target"]]).to(DEV)
    want = render.render_labels(hip.argmax_labels_u16(run["logit_on"]), render.bev_view(dims, 8, device=DEV), (512, 512),
                                fov=torch.stack(run["batch"]["fov_mask_1"]).reshape((run["B"],) + dims),
                                target=target.to(torch.uint8), mode="error", palette="kitti")
    for i in range(run["B"]):
        img = decode_png(str(tmp_path / "err" / "08" / ("%06d_bev.png" % (5 * i))))
        assert np.array_equal(img, want[i, 0].cpu().numpy())
