"""Raw SemanticKITTI voxel files -> labels (occdepth_amd/targets.py: kitti_remap_lut, kitti_labels, read_raw_kitti_voxels;
csrc/targets.hip: occd_kitti_labels), the parts that need no GPU, against tests/golden/kitti_raw_labels.npz -- what the
reference's own readers, remap table, masking and _downsample_label give for synthetic raw files
(tests/golden/make_golden_raw_labels.py).  `emulate_kitti_labels` restates the entry point's contract
(include/occdepth_amd.h) in torch; tests/test_kitti_labels_gpu.py holds the kernel to the same fixture."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kitti_raw_labels.npz")
CASES = {"g16": (1, (16, 16, 16)), "g8x24": (1, (8, 24, 8)), "g32b2": (2, (32, 32, 16))}


def gold():
    return np.load(GOLDEN)


def emulate_kitti_labels(raw, invalid_bits, occluded_bits, lut):
    """occd_kitti_labels on flat (B, N) / (B, N / 8) tensors of any device: -> (target (B, N) uint8, occluded (B, N) uint8
    or None, number of raw values >= len(lut)).  Voxel 8k + j takes bit 7 - j of mask byte k."""
    r = raw.view(torch.int16).to(torch.int64) & 0xFFFF               # the file's 16 bits, whatever the tensor calls them
    table = torch.as_tensor(lut).to(torch.int64)
    known = r < table.numel()
    target = torch.where(known, table[r.clamp(max=table.numel() - 1)], torch.full_like(r, 255))
    shifts = torch.arange(7, -1, -1, dtype=torch.int64)

    def unpack(bits):
        return ((bits.to(torch.int64)[..., None] >> shifts) & 1).reshape(bits.shape[0], -1)

    target = torch.where(unpack(invalid_bits) == 1, torch.full_like(target, 255), target).to(torch.uint8)
    occluded = None if occluded_bits is None else unpack(occluded_bits).to(torch.uint8)
    return target, occluded, int((~known).sum())


def test_fixture_regenerates_from_reference_cpu(tmp_path):
    """The fixture is what the reference's functions produce today (skipped where the reference checkout is absent)."""
    from oracle import ref_shims
    if not ref_shims.available():
        pytest.skip("reference checkout not present")
    out = tmp_path / "raw_labels.npz"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tests", "golden", "make_golden_raw_labels.py"), "--out",
                           str(out)])
    new, old = np.load(out), gold()
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        if k != "__meta__":
            assert new[k].dtype == old[k].dtype and np.array_equal(new[k], old[k]), k


def test_fixture_covers_the_cases_cpu():
    g = gold()
    from occdepth_amd import targets
    keys = {raw for raw, _ in targets.KITTI_LEARNING_MAP}
    for name, (frames, scene) in CASES.items():
        n = int(np.prod(scene))
        assert g[f"{name}.raw"].shape == (frames, n) and g[f"{name}.raw"].dtype == np.uint16
        assert g[f"{name}.invalid_bits"].shape == g[f"{name}.occluded_bits"].shape == (frames, n // 8)
        assert g[f"{name}.target_1_1"].shape == (frames,) + scene and g[f"{name}.target_1_1"].dtype == np.float32
        assert g[f"{name}.target_1_8"].shape == (frames,) + tuple(s // 8 for s in scene)
        for f in range(frames):
            assert keys <= set(g[f"{name}.raw"][f].tolist())
            for bits in (g[f"{name}.invalid_bits"][f], g[f"{name}.occluded_bits"][f]):
                assert {0xFF, 0x00, 0x80, 0x01} <= set(bits.tolist())
            t = g[f"{name}.target_1_1"][f].reshape(scene[0] // 8, 8, scene[1] // 8, 8, scene[2] // 8, 8)
            empty = ((t == 0) | (t == 255)).sum(axis=(1, 3, 5))
            assert (empty > 0.95 * 512).any() and (empty <= 0.95 * 512).any()       # both branches of the 95 % rule


def test_remap_lut_is_the_reference_table_cpu():
    from occdepth_amd import targets
    lut, want = targets.kitti_remap_lut(), gold()["lut"]
    assert lut.dtype == np.uint8 and lut.shape == want.shape == (359,)
    assert np.array_equal(lut.astype(np.int64), want.astype(np.int64))
    assert lut[0] == 0 and lut[1] == 255 and lut[52] == 255 and lut[2] == 255 and lut[10] == 1 and lut[259] == 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_contract_emulation_reproduces_reference_cpu(name):
    from occdepth_amd import targets
    g = gold()
    frames, scene = CASES[name]
    raw, inv, occ = (torch.from_numpy(g[f"{name}.{k}"]) for k in ("raw", "invalid_bits", "occluded_bits"))
    for r in (raw, raw.view(torch.int16)):
        target, occluded, bad = emulate_kitti_labels(r, inv, occ, targets.kitti_remap_lut())
        assert bad == 0
        want = g[f"{name}.target_1_1"]
        assert np.array_equal(target.reshape((frames,) + scene).numpy().astype(np.float32), want)
        assert np.array_equal(occluded.reshape((frames,) + scene).numpy(), g[f"{name}.occluded"])
    # the bit order matters to the fixture: LSB-first unpacking gives another volume
    lsb = np.unpackbits(g[f"{name}.occluded_bits"], axis=1, bitorder="little").reshape((frames,) + scene)
    assert not np.array_equal(lsb, g[f"{name}.occluded"])
    planted = raw.clone()
    planted[0, 0], planted[-1, -1] = 359, 65535
    target, _, bad = emulate_kitti_labels(planted, inv, None, targets.kitti_remap_lut())
    assert bad == 2 and int(target[0, 0]) == 255 and int(target[-1, -1]) == 255


def test_kitti_labels_rejects_bad_arguments_cpu():
    from occdepth_amd import targets
    raw = torch.zeros((1, 64), dtype=torch.uint16)
    inv = torch.zeros((1, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):                             # no CPU path
        targets.kitti_labels(raw, inv, scene_size=(4, 4, 4))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        targets.kitti_labels(raw, inv, scene_size=(3, 3, 3))


def test_raw_rows_checks_shapes_and_dtypes_cpu():
    """The shape and dtype checks of kitti_labels, on CPU tensors posing as device tensors."""
    from occdepth_amd import targets

    class OnDevice(torch.Tensor):
        is_cuda = True

    def dev(t):
        return t.as_subclass(OnDevice)

    raw = dev(torch.zeros((2, 64), dtype=torch.int16))
    assert targets._raw_rows(raw, "raw", (torch.uint16, torch.int16)).shape == (2, 64)
    assert targets._raw_rows([raw[0], raw[1]], "raw", (torch.uint16, torch.int16)).shape == (2, 64)
    assert targets._raw_rows(raw[0], "raw", (torch.uint16, torch.int16)).shape == (1, 64)
    with pytest.raises(RuntimeError, match="int16"):
        targets._raw_rows(dev(torch.zeros((2, 64), dtype=torch.int32)), "raw", (torch.uint16, torch.int16))
    with pytest.raises(RuntimeError, match=r"\(2, 8\)"):
        targets._raw_rows(dev(torch.zeros((2, 7), dtype=torch.uint8)), "invalid_bits", (torch.uint8,), (2, 8))
    with pytest.raises(RuntimeError, match="flat row"):
        targets._raw_rows(dev(torch.zeros((2, 4, 2), dtype=torch.uint8)), "invalid_bits", (torch.uint8,))


def test_entry_point_validates_arguments_cpu(hip_lib):
    """Host-side checks only: invalid arguments return the error status before anything is launched."""
    import ctypes
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15                                       # 16-byte aligned scratch
    args = dict(raw=p, inv=p, occ=None, lut=p, lut_len=359, target=p, occluded=None, count=p, batch=1, N=64)

    def call(**over):
        a = dict(args, **over)
        return hip_lib.occd_kitti_labels(a["raw"], a["inv"], a["occ"], a["lut"], a["lut_len"], a["target"], a["occluded"],
                                         a["count"], a["batch"], a["N"], None)

    assert call(N=60) == -1                                                      # N % 8
    assert call(N=0) == -1 and call(batch=0) == -1
    assert call(raw=None) == -1 and call(inv=None) == -1 and call(lut=None) == -1 and call(target=None) == -1
    assert call(count=None) == -1
    assert call(lut_len=0) == -1 and call(lut_len=4097) == -1
    assert call(occ=p) == -1 and call(occluded=p) == -1                          # the occluded pair comes together
    assert call(raw=p + 1) == -1                                                 # labels are 2-byte values
    assert call(target=p + 4) == -1 and call(occ=p, occluded=p + 2) == -1        # 8-byte stores


def _model_stand_in(gpu_targets="auto", occluded_cls=False, dataset="kitti"):
    """What OccDepth._step_labels reads of the model, with the torch emulation in place of the GPU decode."""
    from occdepth_amd.models.OccDepth import OccDepth
    calls = []

    def kitti_labels(raw, invalid_bits, occluded_bits=None, *, scene_size, lut=None, check=False):
        from occdepth_amd import targets
        assert not check                                                         # the step never reads the counter back
        calls.append(tuple(scene_size))
        raw, invalid_bits, occluded_bits = (torch.stack(list(x)) if isinstance(x, (list, tuple)) else x
                                            for x in (raw, invalid_bits, occluded_bits))
        t, o, _ = emulate_kitti_labels(raw, invalid_bits, occluded_bits, targets.kitti_remap_lut())
        shape = (raw.shape[0],) + tuple(scene_size)
        return t.reshape(shape) if o is None else (t.reshape(shape), o.reshape(shape))

    m = types.SimpleNamespace(gpu_targets=gpu_targets, occluded_cls=occluded_cls, dataset=dataset, project_scale=2,
                              full_scene_size=(32, 32, 16), _tables_absent=OccDepth._tables_absent,
                              _targets=lambda: types.SimpleNamespace(kitti_labels=kitti_labels))
    return m, calls, OccDepth._step_labels


def test_step_labels_key_handling_cpu():
    g = gold()
    raw, inv, occ = (torch.from_numpy(g[f"g32b2.{k}"]) for k in ("raw", "invalid_bits", "occluded_bits"))
    want = torch.from_numpy(g["g32b2.target_1_1"]).to(torch.uint8)
    want_occ = torch.from_numpy(g["g32b2.occluded"])
    raw_keys = dict(voxel_label_raw=raw.view(torch.int16), voxel_invalid_bits=inv, voxel_occluded_bits=occ)
    # raw keys, no target: decoded at the output grid; the batch is left as it was
    m, calls, step_labels = _model_stand_in()
    batch = dict(raw_keys)
    target, occluded = step_labels(m, batch, "cpu")
    assert calls == [(32, 32, 16)] and torch.equal(target, want) and occluded is None
    assert sorted(batch) == sorted(raw_keys)
    # ... as lists of per-sample rows, and with the empty stand-ins of a hooked collate for `target`
    for stub in ([], torch.zeros(0, dtype=torch.uint8)):
        lists = {k: list(v) for k, v in raw_keys.items()}
        target, _ = step_labels(m, dict(lists, target=stub), "cpu")
        assert torch.equal(target, want)
    # occluded_cls: the occluded volume comes from the bits, when the batch has them
    m, calls, step_labels = _model_stand_in(occluded_cls=True)
    target, occluded = step_labels(m, dict(raw_keys), "cpu")
    assert torch.equal(target, want) and torch.equal(occluded, want_occ)
    target, occluded = step_labels(m, {k: v for k, v in raw_keys.items() if k != "voxel_occluded_bits"}, "cpu")
    assert torch.equal(target, want) and occluded is None
    # a batch that brings `target` is used as before: nothing is decoded
    m, calls, step_labels = _model_stand_in(occluded_cls=True)
    brought = torch.full((2, 32, 32, 16), 7, dtype=torch.uint8)
    target, occluded = step_labels(m, dict(raw_keys, target=brought, occluded=want_occ), "cpu")
    assert calls == [] and target is brought and occluded is want_occ
    m.occluded_cls = False
    assert step_labels(m, dict(target=brought, occluded=want_occ), "cpu")[1] is None
    # OCCDEPTH_GPU_TARGETS=0: raw files cannot stand in for `target`
    m, calls, step_labels = _model_stand_in(gpu_targets=False)
    with pytest.raises(RuntimeError, match="OCCDEPTH_GPU_TARGETS"):
        step_labels(m, dict(raw_keys), "cpu")
    assert step_labels(m, dict(raw_keys, target=brought), "cpu")[0] is brought
    # neither `target` nor raw files; another dataset
    m, calls, step_labels = _model_stand_in()
    with pytest.raises(KeyError, match="voxel_label_raw"):
        step_labels(m, dict(img=torch.zeros(1)), "cpu")
    m, calls, step_labels = _model_stand_in(dataset="NYU")
    with pytest.raises(NotImplementedError):
        step_labels(m, dict(raw_keys), "cpu")


def test_batch_signature_and_copy_keep_16_bit_rows_cpu():
    """The raw tensors are static batch entries like any other: the signature tells uint16 from int16, and _copy_batch /
    GraphedTrainStep.load_batch copy them bit for bit."""
    from occdepth_amd.models.OccDepth import OccDepth
    from occdepth_amd.train_graph import GraphedTrainStep
    g = gold()
    raw = torch.from_numpy(g["g32b2.raw"])
    inv = torch.from_numpy(g["g32b2.invalid_bits"])
    for view in (lambda t: t, lambda t: t.view(torch.int16)):
        src = dict(voxel_label_raw=view(raw), voxel_invalid_bits=inv)
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        assert OccDepth._batch_signature(src) == OccDepth._batch_signature(dst)
        OccDepth._copy_batch(dst, src)
        assert all(torch.equal(dst[k].view(torch.uint8), src[k].view(torch.uint8)) for k in src)
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        GraphedTrainStep.load_batch(types.SimpleNamespace(batch=dst), src)
        assert all(torch.equal(dst[k].view(torch.uint8), src[k].view(torch.uint8)) for k in src)
    assert OccDepth._batch_signature(dict(voxel_label_raw=raw)) != \
        OccDepth._batch_signature(dict(voxel_label_raw=raw.view(torch.int16)))


def test_read_raw_kitti_voxels_round_trips_cpu(tmp_path):
    from occdepth_amd import targets
    g = gold()
    raw, inv, occ = (g[f"g8x24.{k}"][0] for k in ("raw", "invalid_bits", "occluded_bits"))
    raw.tofile(tmp_path / "000007.label")
    inv.tofile(tmp_path / "000007.invalid")
    got = targets.read_raw_kitti_voxels(str(tmp_path), "000007")
    assert len(got) == 2 and got[0].dtype == np.uint16 and got[1].dtype == np.uint8
    assert np.array_equal(got[0], raw) and np.array_equal(got[1], inv)
    with pytest.raises(FileNotFoundError):
        targets.read_raw_kitti_voxels(str(tmp_path), "000007", occluded=True)
    occ.tofile(tmp_path / "000007.occluded")
    got = targets.read_raw_kitti_voxels(str(tmp_path), "000007", occluded=True)
    assert len(got) == 3 and got[2].dtype == np.uint8 and np.array_equal(got[2], occ)
    assert torch.from_numpy(got[0]).dtype == torch.uint16                        # what a collate stacks
