"""Training targets built on the GPU (occdepth_amd/targets.py, csrc/targets.hip) against the reference's own dataloader
functions (tests/golden/train_targets.npz, written by tests/golden/make_golden_targets.py):
  frustum masks / class counts   compute_local_frustums   occdepth/data/utils/helpers.py:183-260
  1:8 labels                     _downsample_label        occdepth/data/NYU/preprocess.py:102-143
  relation matrices              compute_CP_mega_matrix   occdepth/data/utils/helpers.py:6-91
bit for bit, and `OccDepth.step` / the captured training step on a batch that brings none of them."""
import ctypes
import os
import subprocess
import sys
import types
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "train_targets.npz")
TARGET_KEYS = ("frustums_masks", "frustums_class_dists", "CP_mega_matrices")


def gold():
    return np.load(GOLDEN)


def unpack(g, bits_key, shape):
    shape = tuple(int(s) for s in shape)
    return np.unpackbits(g[bits_key])[:int(np.prod(shape))].reshape(shape).astype(bool)


def geometry(case):
    g = gold()
    return dict(vox_origin=(0.0, -25.6, -2.0), voxel_size=0.2, img_wh=(1220, 370), frustum_size=8, n_classes=20) \
        if case == "full" else \
        dict(vox_origin=(0.0, -6.4, -2.0), voxel_size=0.2, img_wh=(320, 96), frustum_size=8, n_classes=20), g


# ------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_regenerates_from_reference_cpu(tmp_path):
    """The fixture is what the reference's functions produce today (skipped where the reference checkout is absent)."""
    from oracle import ref_shims
    if not ref_shims.available():
        pytest.skip("reference checkout not present")
    out = tmp_path / "targets.npz"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_targets.py"), "--out",
                           str(out)])
    new, old = np.load(out), gold()
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if k != "__meta__":
            assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k


def test_defer_dataset_targets_rebinds_and_undoes_cpu():
    from occdepth_amd import targets

    def frustums(*a, **k):
        return "masks", "dists"

    def cp(*a, **k):
        return "cp"

    mod = types.ModuleType("stand_in_kitti_dataset")
    mod.compute_local_frustums, mod.compute_CP_mega_matrix, mod.other = frustums, cp, 7
    hook = targets.defer_dataset_targets(mod)
    assert hook.active
    assert mod.compute_local_frustums is not frustums and mod.compute_CP_mega_matrix is not cp and mod.other == 7
    m, d = mod.compute_local_frustums(np.zeros((2, 8, 1, 2)), np.zeros((2, 8)), np.zeros((2, 2, 2)), 1220, 370,
                                      dataset="kitti", n_classes=20, size=8)
    assert m is None and d is None                                  # the reference collate skips None masks
    z = mod.compute_CP_mega_matrix(np.zeros((32, 32, 4), dtype=np.uint8))
    assert isinstance(z, np.ndarray) and z.dtype == np.uint8 and z.size == 0
    t = torch.from_numpy(z)                                         # what the collate does with it
    assert t.dtype == torch.uint8 and t.numel() == 0
    again = targets.defer_dataset_targets(mod)                      # already stubbed: nothing more to rebind
    assert not again.active
    hook.undo()
    assert mod.compute_local_frustums is frustums and mod.compute_CP_mega_matrix is cp
    hook.undo()                                                     # idempotent
    assert mod.compute_local_frustums is frustums
    with targets.defer_dataset_targets(mod):
        assert mod.compute_CP_mega_matrix is not cp
    assert mod.compute_CP_mega_matrix is cp


def test_defer_dataset_targets_without_reference_module_cpu(monkeypatch):
    from occdepth_amd import targets
    monkeypatch.setattr(targets, "KITTI_DATASET_MODULE", "occdepth_amd_no_such_module.kitti_dataset")
    hook = targets.defer_dataset_targets()
    assert not hook.active
    hook.undo()


def test_target_entry_points_validate_arguments_cpu(hip_lib, tmp_path):
    """Host-side checks only (no launch for invalid arguments), and the args struct has the C layout."""
    from occdepth_amd import hip
    assert hip_lib.occd_frustum_targets(None, None) == -1
    a = hip.FrustumArgs()
    assert hip_lib.occd_frustum_targets(ctypes.byref(a), None) == -1
    assert hip_lib.occd_downsample_label(None, None, 1, 8, 8, 8, 8, None) == -1
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert hip_lib.occd_downsample_label(p, p, 1, 12, 8, 8, 8, None) == -1      # 12 is not a multiple of 8
    assert hip_lib.occd_cp_mega_matrix(p, p, 1, 1, 8, 8, 0, None) == -1         # no mega voxel along x
    assert hip_lib.occd_cp_mega_matrix(None, p, 1, 8, 8, 8, 0, None) == -1
    hdr = os.path.join(ROOT, "include", "occdepth_amd.h")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hdr}"', "int main(void){",
             'printf("size %zu\\n", sizeof(occd_frustum_args));']
    lines += [f'printf("{n} %zu\\n", offsetof(occd_frustum_args, {n}));' for n, _ in hip.FrustumArgs._fields_]
    lines += ["return 0;}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(got["size"]) == ctypes.sizeof(hip.FrustumArgs)
    for n, _ in hip.FrustumArgs._fields_:
        assert int(got[n]) == getattr(hip.FrustumArgs, n).offset, n


# ------------------------------------------------------------------------------------------------------------ GPU
def _run_frustums(case, views, ext_dtype=torch.float64):
    from occdepth_amd import targets
    geo, g = geometry(case)
    E = torch.from_numpy(g[f"{case}.cam_E"][views]).to(ext_dtype).double()[None].cuda()
    K = torch.from_numpy(g[f"{case}.cam_k"][views])[None].cuda()
    tgt = torch.from_numpy(g[f"{case}.target"])[None].cuda()
    masks, dists = targets.frustum_targets(E, K, tgt, **geo)
    return masks, dists, g


def _digests(masks):
    """(F, X, Y, Z) bool GPU tensor -> the fixture's per-frustum (count, index sum, CRC32 of packbits)."""
    flat = masks.reshape(masks.shape[0], -1)
    idx = torch.arange(flat.shape[1], device=flat.device, dtype=torch.int64)
    cnt = flat.sum(1).cpu().numpy()
    isum = (flat.to(torch.int64) * idx).sum(1).cpu().numpy()
    host = flat.cpu().numpy()
    return np.stack([cnt, isum, np.array([zlib.crc32(np.packbits(r).tobytes()) for r in host])], 1).astype(np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,views", [("stereo", [0, 1]), ("left", [0])])
def test_frustum_targets_full_size_bit_exact_gpu(hip_lib, tag, views):
    masks, dists, g = _run_frustums("full", views)
    assert masks.dtype == torch.bool and tuple(masks.shape) == (1, 64, 256, 256, 32) and tuple(dists.shape) == (1, 64, 20)
    want = g[f"full.{tag}.mask_digest"]
    got = _digests(masks[0])
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))
    assert np.array_equal(dists[0].cpu().double().numpy(), g[f"full.{tag}.dists"])
    assert int(want[:, 0].sum()) > 10 ** 6                               # the masks are not trivially empty


@pytest.mark.gpu
@pytest.mark.parametrize("tag,views", [("stereo", [0, 1]), ("left", [0])])
def test_frustum_targets_small_bit_exact_gpu(hip_lib, tag, views):
    masks, dists, g = _run_frustums("small", views)
    want = unpack(g, f"small.{tag}.mask_bits", g[f"small.{tag}.mask_shape"])
    assert np.array_equal(masks[0].cpu().numpy(), want)
    assert np.array_equal(dists[0].cpu().double().numpy(), g[f"small.{tag}.dists"])


@pytest.mark.gpu
def test_frustum_targets_float32_extrinsics_gpu(hip_lib):
    """The batch's float32 copy of the extrinsics moves a few voxels by one pixel: at most 1e-4 of them change frustum."""
    m64, _, _ = _run_frustums("full", [0, 1])
    m32, _, _ = _run_frustums("full", [0, 1], ext_dtype=torch.float32)
    differ = int((m64[0] != m32[0]).any(0).sum())
    n = m64[0, 0].numel()
    print("voxels whose membership differs with float32 extrinsics:", differ, "of", n)
    assert differ <= 1e-4 * n


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["full", "small"])
def test_downsample_and_cp_matrix_bit_exact_gpu(hip_lib, case):
    from occdepth_amd import targets
    g = gold()
    tgt = torch.from_numpy(g[f"{case}.target"]).cuda()
    t18 = targets.downsample_label(tgt[None], 8)
    assert np.array_equal(t18[0].cpu().numpy(), g[f"{case}.target_1_8"])
    assert np.array_equal(targets.downsample_label(tgt, 8).cpu().numpy(), g[f"{case}.target_1_8"])
    coarse = torch.from_numpy(g[f"{case}.target_1_8"]).cuda()[None]
    for tag, binary in (("cp4", False), ("cp2", True)):
        cp = targets.cp_mega_matrix(coarse, binary=binary)
        shape = tuple(int(s) for s in g[f"{case}.{tag}.shape"])
        assert cp.dtype == torch.uint8 and tuple(cp.shape) == (1,) + shape
        assert np.array_equal(cp[0].cpu().numpy(), unpack(g, f"{case}.{tag}.bits", shape).astype(np.uint8)), tag


def _small_batch():
    """kitti_small model + batch (test_train_step._small_train_setup, with the down-scaled classifier convolutions of the
    train_step_small fixture so no loss term overflows) on the fixture's "mixed" target, with the calibration's float64
    extrinsics and the reference's targets for that target."""
    from test_oracle_vs_golden import gold as gold_step
    from test_train_step import _small_train_setup
    g = gold()
    m, batch = _small_train_setup("kitti_small", "cuda")
    gs = gold_step("train_step_small")
    over = {f[len("kitti_small") + 10:]: torch.from_numpy(gs[f]) for f in gs.files if f.startswith("kitti_small.override.")}
    assert over
    m.load_state_dict({k: v.cuda() for k, v in over.items()}, strict=False)
    assert np.array_equal(batch["target"][0].cpu().numpy(), g["small.target"])
    batch["target"] = torch.from_numpy(g["mixed.target"])[None].cuda()
    batch["T_velo_2_cam_f64"] = [torch.from_numpy(g["small.cam_E"]).cuda()]
    masks = unpack(g, "mixed.stereo.mask_bits", g["mixed.stereo.mask_shape"])
    batch["frustums_masks"] = [torch.from_numpy(masks).cuda()]
    batch["frustums_class_dists"] = [torch.from_numpy(g["mixed.stereo.dists"]).float().cuda()]
    cp = unpack(g, "mixed.cp4.bits", g["mixed.cp4.shape"]).astype(np.uint8)
    batch["CP_mega_matrices"] = [torch.from_numpy(cp).cuda()]
    return m, batch


@pytest.mark.gpu
def test_step_builds_missing_targets_gpu(hip_lib):
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    m, full = _small_batch()
    m = m.eval()
    assert m.gpu_targets == "auto" and m.fp_loss and m.context_prior and m.relation_loss
    stripped = {k: v for k, v in full.items() if k not in TARGET_KEYS}
    empty = dict(stripped, frustums_masks=[], frustums_class_dists=[],
                 CP_mega_matrices=[torch.zeros(0, dtype=torch.uint8, device="cuda")])   # what the hooked collate gives
    logged = {}
    for name, batch in (("reference", full), ("stripped", stripped), ("empty", empty)):
        m.cur_batch = 3
        with torch.no_grad():
            m.step(batch, "train", SSCMetrics(m.n_classes, device="cuda"))
        logged[name] = {k: float(v) for k, v in m.logged.items()}
        with torch.no_grad():
            m.step(batch, "val", None)
        logged[name + "/val"] = {k: float(v) for k, v in m.logged.items()}
    print(logged)
    # what the step builds is the reference's targets, bit for bit
    bm, bd = m.frustum_targets_on_gpu(stripped, stripped["target"])
    assert torch.equal(bm[0], full["frustums_masks"][0]) and torch.equal(bd[0], full["frustums_class_dists"][0])
    assert torch.equal(m.relation_targets_on_gpu(stripped["target"])[0], full["CP_mega_matrices"][0])
    assert all(np.isfinite(v) for v in logged["reference"].values()), logged["reference"]
    for name in ("stripped", "empty"):
        for suffix in ("", "/val"):
            ref, got = logged["reference" + suffix], logged[name + suffix]
            assert sorted(ref) == sorted(got)
            assert any(k.endswith("loss_frustums") for k in ref) and any(k.endswith("loss_relation_ce_super") for k in ref)
            for k in ref:
                assert got[k] == pytest.approx(ref[k], rel=1e-6, abs=1e-12), (name, k)
    m.gpu_targets = False
    with pytest.raises(KeyError):
        with torch.no_grad():
            m.step(stripped, "train", None)


@pytest.mark.gpu
def test_whole_step_hipgraph_builds_targets_gpu(hip_lib):
    """GraphedTrainStep on a target-free batch captures the builders with the step; replays match eager steps fed the
    reference's targets (the tolerances of test_train_step.test_whole_step_hipgraph_matches_eager_gpu)."""
    import copy
    from occdepth_amd import train_graph
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    m0, full = _small_batch()
    stripped = {k: v for k, v in full.items() if k not in TARGET_KEYS}
    runs = {}
    for mode, batch in (("eager", full), ("graph", stripped)):
        m = copy.deepcopy(m0).train()
        m.cur_batch = 0
        opt = train_graph.make_capturable(torch.optim.AdamW(m.parameters(), lr=1e-4, fused=True))
        gs = train_graph.GraphedTrainStep(m, opt, batch, warmup=2)
        if mode == "graph":
            assert gs.capture(), gs.error
            assert not any(k in gs.batch for k in TARGET_KEYS)
        losses = [float(gs()) for _ in range(3)]
        terms = {k: float(v) for k, v in m.logged.items()}
        runs[mode] = (losses, terms, next(iter(m.net_3d_decoder.parameters())).detach().float().cpu().clone())
    (le, te, pe), (lg, tg, pg) = runs["eager"], runs["graph"]
    print("eager", le, "graph", lg)
    assert any(k.endswith("loss_frustums") for k in tg) and sorted(te) == sorted(tg)
    assert abs(le[0] - lg[0]) <= 1e-5 * abs(le[0]), (le, lg)
    assert all(abs(a - b) <= 1.5e-2 * abs(a) for a, b in zip(le, lg)), (le, lg)
    assert float((pe - pg).abs().max() / pe.abs().max()) < 5e-3
