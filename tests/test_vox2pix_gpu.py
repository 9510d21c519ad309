"""The reference dataset's voxel -> pixel tables built on the GPU (occd_vox2pix: batched, device calibration, flip-aware)
and the model paths that use them when a batch brings no tables: the training lift (eager and captured), the eval lift
(in-kernel projection with the flip of ida_mats) and `project_voxels_on_gpu`."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TABLES = ("projected_pix_2", "fov_mask_2")


def _kitti_E():
    from oracle import inputs
    tr2 = inputs.KITTI_TR.copy()
    tr2[0, 3] = -0.54
    return np.stack([inputs.KITTI_TR, tr2])


def _flip_ida(W):
    """img_transform((0, 0, W, H), flip=True) of kitti_dataset.py:20-37."""
    m = torch.eye(4)
    m[0, 0] = -1.0
    m[0, 3] = float(W)
    return m


# ----------------------------------------------------------------------------------------------------------- kernel
GRIDS = {
    # name: (scene metres, voxel metres, image (W, H), intrinsics scale, origin)
    "config2_project_scale": ((51.2, 51.2, 6.4), 0.4, (1220, 370), 1.0, (0.0, -25.6, -2.0)),
    "output_scale": ((51.2, 51.2, 6.4), 0.2, (1220, 370), 1.0, (0.0, -25.6, -2.0)),
    "kitti_small": ((12.8, 12.8, 3.2), 0.4, (320, 96), 320 / 1220, (0.0, -6.4, -2.0)),
    "non_pow2_60x36x60": ((15.0, 9.0, 15.0), 0.25, (1220, 370), 1.0, (0.0, -4.5, -2.0)),
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_vox2pix_bit_exact_with_mixed_flips_gpu(hip_lib, name):
    """B = 2, V = 2 in one launch, (0, 1) and (1, 0) flipped: every entry equals hip.project_voxels per (b, v) with the
    flip applied in torch; FOV masks and in-FOV pixels equal the numpy restatement of the reference's vox2pix."""
    from occdepth_amd import hip
    from oracle import inputs
    scene, vs, (W, H), ks, origin = GRIDS[name]
    dims = tuple(int(d) for d in np.ceil(np.asarray(scene) / vs))
    K = inputs.KITTI_K.copy()
    K[:2] *= ks
    E = np.stack([_kitti_E(), _kitti_E()])
    E[1, :, :3, 3] += np.array([0.05, -0.03, 0.02])                  # the second sample has its own extrinsics
    Kb = np.stack([np.stack([K, K])] * 2)
    Kb[1, :, 0, 0] *= 1.01
    flips = [[False, True], [True, False]]
    ida = torch.stack([torch.stack([_flip_ida(W) if f else torch.eye(4) for f in row]) for row in flips]).to(DEV)
    Ed, Kd = torch.from_numpy(E).to(DEV), torch.from_numpy(Kb).to(DEV)
    pix, fov, z = hip.vox2pix(Ed, Kd, ida.contiguous(), origin, vs, dims, (W, H), with_z=True)
    n = dims[0] * dims[1] * dims[2]
    assert pix.shape == (2, 2, n, 1, 2) and pix.dtype == torch.int64 and fov.shape == (2, 2, n, 1) and fov.dtype == torch.bool
    nf, nz = hip.vox2pix(Ed, Kd, None, origin, vs, dims, (W, H))
    for b in range(2):
        for v in range(2):
            rp, rf, rz = hip.project_voxels(E[b, v], Kb[b, v], origin, vs, dims, W, H, with_z=True)
            if flips[b][v]:
                rp = rp.clone()
                rp[..., 0] = W - 1 - rp[..., 0]
            assert torch.equal(pix[b, v], rp) and torch.equal(fov[b, v], rf), (b, v)
            assert torch.equal(z[b, v], rz), (b, v)
            assert torch.equal(nf[b, v][..., 1], pix[b, v][..., 1]) and torch.equal(nz[b, v], fov[b, v])
            op, of, _ = inputs.vox2pix(E[b, v], Kb[b, v], origin, vs, W, H, scene, 0)
            if flips[b][v]:
                op[:, :, 0] = W - 1 - op[:, :, 0]
            assert np.array_equal(fov[b, v].cpu().numpy(), of), (b, v)
            inside = of[:, 0]
            assert np.array_equal(pix[b, v].cpu().numpy()[inside], op[inside]), (b, v)
            assert 0.02 < inside.mean() < 0.98, inside.mean()


def test_vox2pix_float32_extrinsics_gpu(hip_lib):
    """What a hooked loader projects with: the reference collate keeps only the float32 copy of the extrinsics.  At
    config 2 (project scale and output scale, the golden targets' calibration) at most 1e-4 of the voxels move."""
    import os
    from occdepth_amd import hip
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_targets.npz"))
    E64 = torch.from_numpy(g["full.cam_E"]).double()[None].to(DEV).contiguous()
    K = torch.from_numpy(g["full.cam_k"]).double()[None].to(DEV).contiguous()
    E32 = E64.float().double()
    for vs, dims in ((0.4, (128, 128, 16)), (0.2, (256, 256, 32))):
        p64, f64 = hip.vox2pix(E64, K, None, (0.0, -25.6, -2.0), vs, dims, (1220, 370))
        p32, f32 = hip.vox2pix(E32, K, None, (0.0, -25.6, -2.0), vs, dims, (1220, 370))
        moved = ((f64 != f32) | ((p64 != p32).any(-1) & f64 & f32)).sum()
        n = f64[0, 0].numel()
        print(f"voxel {vs} m: {int(moved)} in-FOV (view, voxel) entries of {f64.numel()} differ with float32 extrinsics")
        assert int(moved) <= 1e-4 * n


# ------------------------------------------------------------------------------------------------------- model paths
def _train_setup():
    """kitti_small model (the down-scaled classifier convolutions of the train_step_small fixture, as
    test_train_targets) + its batch with the float64 extrinsics its tables were projected with."""
    from test_oracle_vs_golden import gold as gold_step
    from test_train_step import _small_train_setup
    m, batch = _small_train_setup("kitti_small", DEV)
    gs = gold_step("train_step_small")
    over = {f[len("kitti_small") + 10:]: torch.from_numpy(gs[f]) for f in gs.files if f.startswith("kitti_small.override.")}
    assert over
    m.load_state_dict({k: v.to(DEV) for k, v in over.items()}, strict=False)
    batch["T_velo_2_cam_f64"] = [torch.from_numpy(_kitti_E()).to(DEV) for _ in batch["cam_k"]]
    assert all(k in batch for k in TABLES)
    return m, batch


def _without(batch):
    return {k: v for k, v in batch.items() if k not in TABLES}


def _zero_size(batch):
    n = len(batch["cam_k"])
    V = batch["cam_k"][0].shape[0]
    return dict(_without(batch), projected_pix_2=[torch.zeros((V, 0, 1, 2), dtype=torch.int64, device=DEV)] * n,
                fov_mask_2=[torch.zeros((V, 0, 1), dtype=torch.bool, device=DEV)] * n)


def _flipped(batch):
    """The reference's flip augmentation applied to a batch: images along W, ida_mats, the tables' x (:388)."""
    W = batch["img"].shape[-1]
    out = dict(batch, img=batch["img"].flip(-1).contiguous(),
               ida_mats=[_flip_ida(W).repeat(t.shape[0], 1, 1).to(t.device) for t in batch["ida_mats"]])
    pix = []
    for p in batch["projected_pix_2"]:
        q = p.clone()
        q[..., 0] = W - 1 - q[..., 0]
        pix.append(q)
    out["projected_pix_2"] = pix
    return out


def _step(m, batch):
    """One training step of the reference's loss assembly (training mode, fixed seed) -> ssc_logit, the logged loss
    terms and the flat parameter gradients."""
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    m.train()
    m.zero_grad(set_to_none=True)
    m.cur_batch = 3
    torch.manual_seed(0)
    logit = m(batch)["ssc_logit"].detach().clone()
    torch.manual_seed(0)
    loss = m.step(batch, "train", SSCMetrics(m.n_classes, device=DEV))
    loss.backward()
    terms = {k: float(v) for k, v in m.logged.items()}
    grads = torch.cat([p.grad.detach().double().flatten() for _, p in sorted(m.named_parameters()) if p.grad is not None])
    return logit, terms, grads


def _check_table_free_steps(m, fed, variants):
    """Every variant's step equals the table-fed step: logits and loss terms within the spread of three table-fed runs
    (identical when that spread is 0; the terms at least to rel 1e-6), gradients within the spread of the table-fed runs
    (the lift backward scatters with float atomics)."""
    runs = [_step(m, fed) for _ in range(3)]
    l0, t0, g0 = runs[0]
    lspread = max(float((l - l0).abs().max()) for l, _, _ in runs[1:])
    tspread = {k: max(abs(t[k] - t0[k]) for _, t, _ in runs[1:]) for k in t0}
    spread = max(float((g - g0).abs().max()) for _, _, g in runs[1:])
    scale = float(g0.abs().max())
    print("table-fed spreads: logits", lspread, "gradients", spread, "of", scale, "terms", tspread)
    assert all(np.isfinite(v) for v in t0.values()) and any(k.endswith("loss_frustums") for k in t0)
    for name, batch in variants.items():
        l, t, g = _step(m, batch)
        lerr = float((l - l0).abs().max())
        err = float((g - g0).abs().max())
        print(name, "logit difference", lerr, "gradient difference", err)
        assert lerr <= 4 * lspread, (name, lerr, lspread)
        assert sorted(t) == sorted(t0), name
        for k in t0:
            assert abs(t[k] - t0[k]) <= max(1e-6 * abs(t0[k]), 4 * tspread[k], 1e-12), (name, k, t[k], t0[k])
        assert g.shape == g0.shape and err <= 4 * spread + 1e-7 * scale, (name, err, spread)


def test_training_step_without_tables_gpu(hip_lib):
    """The step on a batch without tables (keys removed, or zero-size tables) builds them on the GPU and equals the step
    fed the loader's tables.  Without the feature the table-free step raises KeyError."""
    m, full = _train_setup()
    built_pix, built_fov = m.project_voxels_on_gpu(_without(full), full["img"])
    assert torch.equal(built_pix, torch.stack(full["projected_pix_2"])) and torch.equal(built_fov, torch.stack(full["fov_mask_2"]))
    _check_table_free_steps(m, full, {"no keys": _without(full), "zero-size": _zero_size(full)})


def test_training_step_flipped_without_tables_gpu(hip_lib):
    """A flipped batch (images, ida_mats and tables flipped as the reference's loader does): the table-free step builds
    the flipped tables and equals the table-fed step; the eval in-kernel lift honours the flip."""
    from occdepth_amd import hip
    m, full = _train_setup()
    m = m.eval()
    flipped = _flipped(full)
    built_pix, built_fov = m.project_voxels_on_gpu(_without(flipped), flipped["img"])
    assert torch.equal(built_pix, torch.stack(flipped["projected_pix_2"]))
    assert torch.equal(built_fov, torch.stack(flipped["fov_mask_2"]))
    _check_table_free_steps(m, flipped, {"flipped, no keys": _without(flipped), "flipped, zero-size": _zero_size(flipped)})
    m.eval()
    # eval: in-kernel lift on the flipped table-free batch against the table path on the flipped tables
    with torch.no_grad(), hip.profile() as prof:
        o_k = m(_without(flipped))
        torch.cuda.synchronize()
    tags = {k.split(":")[0] for k in prof.rows}
    assert "sfa_lift_proj" in tags and "sfa_lift" not in tags, sorted(tags)
    with torch.no_grad():
        o_t = m(flipped)
        o_nf = m(dict(_without(flipped), ida_mats=full["ida_mats"]))       # the same images lifted WITHOUT the flip
    scale = o_t["ssc_logit"].abs().max()
    err = float((o_k["ssc_logit"] - o_t["ssc_logit"]).abs().max() / scale)
    miss = float((o_nf["ssc_logit"] - o_t["ssc_logit"]).abs().max() / scale)
    print("flipped eval: in-kernel vs table path", err, "; ignoring the flip", miss)
    assert err < 5e-4                 # the two lift kernels differ by <= 3 ulp (tests/test_lift_proj.py), nothing more
    assert miss > 100 * max(err, 1e-7)


def test_lift_proj_flip_and_identity_gpu(hip_lib):
    """occd_lift_proj_fwd: identity idas give the null-ida outputs bit for bit; a mixed flip gathers exactly what the
    table lift gathers through occd_vox2pix's flipped tables (to the 1e-6 bar of tests/test_lift_proj.py)."""
    from test_lift_proj import build_case
    from occdepth_amd import hip
    from occdepth_amd.hip import Vox
    B, V, C, scales, dims, (H, W) = 2, 2, 32, (1, 2), (64, 64, 8), (185, 610)
    feats, _, _, cam, frustum, voxel = build_case(hip, B, V, C, scales, dims, (H, W), True)
    strides = (dims[1] * dims[2], dims[2], 1)
    origin = (0.0, -25.6, -2.0)

    def proj(ida):
        out = Vox.empty(B, dims, C, DEV)
        out.buf.fill_(float("nan"))
        hip.lift_proj(feats, scales, cam[0], cam[1], origin, voxel, (W, H), dims, strides, out, frustum=frustum, ida=ida)
        return out.buf

    eye = torch.eye(4, device=DEV).repeat(B, V, 1, 1).contiguous()
    plain = proj(None)
    assert torch.equal(proj(eye), plain)
    ida = eye.clone()
    ida[0, 1] = _flip_ida(W).to(DEV)
    ida[1, 0] = _flip_ida(W).to(DEV)
    got = proj(ida)
    pix, fov = hip.vox2pix(cam[0], cam[1], ida, origin, voxel, dims, (W, H))
    ref = Vox.empty(B, dims, C, DEV)
    hip.lift(feats, scales, pix, fov, dims, strides, ref, depth_scale=frustum.sample(), scale_const=100.0)
    err = float((got - ref.buf).abs().max() / ref.buf.abs().max())
    assert err < 1e-6, err
    assert float((got - plain).abs().max() / plain.abs().max()) > 1e-2        # the flip is applied, not ignored


def test_eval_zero_size_tables_equal_no_tables_gpu(hip_lib):
    """Eval: zero-size tables (a hooked loader) reach the in-kernel lift like a batch without the table keys."""
    from occdepth_amd import hip
    m, full = _train_setup()
    m = m.eval()
    with torch.no_grad():
        a = m(_without(full))
        with hip.profile() as prof:
            b = m(_zero_size(full))
            torch.cuda.synchronize()
    assert "sfa_lift_proj" in {k.split(":")[0] for k in prof.rows}
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k


def test_whole_step_hipgraph_without_tables_gpu(hip_lib):
    """GraphedTrainStep on a table-free batch captures the projection with the step; replays match eager steps fed the
    tables (the tolerances of test_train_targets.test_whole_step_hipgraph_builds_targets_gpu)."""
    from occdepth_amd import train_graph
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, full = _train_setup()
    runs = {}
    for mode, batch in (("eager", full), ("graph", _without(full))):
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        opt = train_graph.make_capturable(torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True))
        gs = train_graph.GraphedTrainStep(m, opt, batch, warmup=2)
        if mode == "graph":
            assert gs.capture(), gs.error
            assert not any(k in gs.batch for k in TABLES)
        losses = [float(gs()) for _ in range(3)]
        terms = {k: float(v) for k, v in m.logged.items()}
        runs[mode] = (losses, terms, next(iter(m.net_3d_decoder.parameters())).detach().float().cpu().clone())
    (le, te, pe), (lg, tg, pg) = runs["eager"], runs["graph"]
    print("eager", le, "graph", lg)
    assert sorted(te) == sorted(tg)
    assert abs(le[0] - lg[0]) <= 1e-5 * abs(le[0]), (le, lg)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(le, lg)), (le, lg)
    assert float((pe - pg).abs().max() / pe.abs().max()) < 5e-3
