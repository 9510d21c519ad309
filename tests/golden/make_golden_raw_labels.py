"""Generate tests/golden/kitti_raw_labels.npz: the reference's OWN reading and preprocessing of raw SemanticKITTI voxel
files, on CPU, for synthetic files.

    python tests/golden/make_golden_raw_labels.py [--out PATH] [--time-full]

Runs where the reference checkout exists (not on the GPU machines).  Synthetic `<frame>.label` (uint16), `.invalid` and
`.occluded` (bit-packed) files are written to a temporary directory and taken through the reference's functions:
  _read_label_SemKITTI, _read_invalid_SemKITTI, _read_occluded_SemKITTI, get_remap_lut
                                 occdepth/data/semantic_kitti/io_data.py:10-22,115-134,175-195
  the remap and masking lines    occdepth/data/semantic_kitti/preprocess.py:78-84 (they sit inside its hydra `main`, so they
                                 are applied here to the arrays the functions above return)
  _downsample_label              occdepth/data/NYU/preprocess.py:102-143 (preprocess.py:92-94, the 1:8 labels)
`imageio` (imported by io_data, absent here and unused by these functions), `hydra` and `omegaconf` are stubbed.

Cases (frames x grid):
  g16      1 x (16, 16, 16)
  g8x24    1 x (8, 24, 8)      1536 voxels: no multiple of a workgroup's chunk
  g32b2    2 x (32, 32, 16)    a batch of two frames
Raw labels per frame: every 8^3 block draws a share of zeros (0.97, 0.1, 1.0 or 0.5; the first four blocks of a frame take
them in turn, so the smallest grid has them too) and fills the rest with keys of `learning_map`; about 60 % of the voxels
are zero and zeros come in runs.  Every key of `learning_map` and 0 are then planted once.  Invalid bits are set in about
10 % of the voxels, occluded bits in about 40 %, independently; both masks also get the bytes 0xFF, 0x00, 0x80 (voxel 8k)
and 0x01 (voxel 8k + 7) planted.
Blocks per branch of _downsample_label's 95 % rule, (more than 95 % empty or invalid, labelled majority), as generated:
  g16 (4, 4)    g8x24 (2, 1)    g32b2 (15, 17) and (10, 22)
generate() requires at least one block of each branch in every frame.

--time-full also times the same CPU path once on a 256 x 256 x 32 frame (remap + mask + _downsample_label) and prints it;
tools/bench_kitti_labels.py carries a numpy restatement for the GPU machines, where the reference is absent.
"""
import argparse
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle.ref_shims import REF_ROOT  # noqa: E402

CASES = (("g16", 1, (16, 16, 16)), ("g8x24", 1, (8, 24, 8)), ("g32b2", 2, (32, 32, 16)))
ZERO_SHARES = (0.97, 0.1, 1.0, 0.5)
SHARE_PROBS = (0.2, 0.3, 0.2, 0.3)
YAML = os.path.join(REF_ROOT, "occdepth", "data", "semantic_kitti", "semantic-kitti.yaml")


def import_reference():
    sys.path.insert(0, REF_ROOT)
    for name in ("hydra", "omegaconf", "imageio"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["hydra"].main = lambda *a, **k: (lambda f: f)
    sys.modules["omegaconf"].DictConfig = dict
    import occdepth.data.semantic_kitti.io_data as io_data
    import occdepth.data.NYU.preprocess as nyu_preprocess
    return io_data, nyu_preprocess


def learning_map_keys():
    import yaml
    with open(YAML) as f:
        return sorted(yaml.safe_load(f)["learning_map"].keys())


def synthetic_raw(rng, scene, keys):
    X, Y, Z = scene
    raw = np.zeros(scene, dtype=np.uint16)
    i = 0
    for bx in range(X // 8):
        for by in range(Y // 8):
            for bz in range(Z // 8):
                share = ZERO_SHARES[i] if i < len(ZERO_SHARES) else rng.choice(ZERO_SHARES, p=SHARE_PROBS)
                i += 1
                block = rng.choice(np.asarray(keys, dtype=np.uint16), size=(8, 8, 8))
                block[rng.random((8, 8, 8)) < share] = 0
                raw[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8] = block
    flat = raw.reshape(-1)
    where = rng.choice(flat.size, size=len(keys) + 1, replace=False)
    flat[where] = np.asarray(list(keys) + [0], dtype=np.uint16)
    return flat


def synthetic_bits(rng, n_voxels, share):
    bits = np.packbits(rng.random(n_voxels) < share)                 # MSB first, like io_data.pack
    where = rng.choice(bits.size, size=8, replace=False)
    bits[where] = np.asarray([0xFF, 0x00, 0x80, 0x01, 0xFF, 0x00, 0x80, 0x01], dtype=np.uint8)
    return bits


def reference_labels(io_data, nyu_preprocess, lut, folder, frame, scene):
    """What preprocess.py:76-97 saves for one frame, and the occluded volume of kitti_dataset.py:312-313."""
    base = os.path.join(folder, frame)
    label = io_data._read_label_SemKITTI(base + ".label")
    invalid = io_data._read_invalid_SemKITTI(base + ".invalid")
    occluded = io_data._read_occluded_SemKITTI(base + ".occluded")
    label = lut[label.astype(np.uint16)].astype(np.float32)          # preprocess.py:78-80
    label[np.isclose(invalid, 1)] = 255                               # preprocess.py:81-83
    label = label.reshape(scene)
    return label, nyu_preprocess._downsample_label(label, scene, 8), occluded.reshape(scene)


def branch_counts(target_1_1):
    """(blocks with more than 95 % of 0 / 255, the others) of one frame."""
    X, Y, Z = target_1_1.shape
    t = target_1_1.reshape(X // 8, 8, Y // 8, 8, Z // 8, 8)
    empty = ((t == 0) | (t == 255)).sum(axis=(1, 3, 5))
    first = int((empty > 0.95 * 512).sum())
    return first, int(empty.size - first)


def generate():
    io_data, nyu_preprocess = import_reference()
    keys = learning_map_keys()
    lut = io_data.get_remap_lut(YAML)
    rng = np.random.default_rng(20261018)
    arrays, meta = {"lut": lut}, {"lut_dtype": str(lut.dtype), "cases": {}}
    with tempfile.TemporaryDirectory() as folder:
        for name, frames, scene in CASES:
            n = int(np.prod(scene))
            per = {k: [] for k in ("raw", "invalid_bits", "occluded_bits", "target_1_1", "target_1_8", "occluded")}
            branches = []
            for f in range(frames):
                frame = "%06d" % f
                raw = synthetic_raw(rng, scene, keys)
                inv, occ = synthetic_bits(rng, n, 0.10), synthetic_bits(rng, n, 0.40)
                assert set(keys) | {0} <= set(raw.tolist())
                raw.tofile(os.path.join(folder, frame + ".label"))
                inv.tofile(os.path.join(folder, frame + ".invalid"))
                occ.tofile(os.path.join(folder, frame + ".occluded"))
                t11, t18, occluded = reference_labels(io_data, nyu_preprocess, lut, folder, frame, scene)
                assert t11.dtype == np.float32 and t18.dtype == np.uint8 and occluded.dtype == np.uint8
                b = branch_counts(t11)
                assert min(b) >= 1, (name, f, b)
                branches.append(b)
                for k, v in zip(per, (raw, inv, occ, t11, t18, occluded)):
                    per[k].append(v)
            for k, v in per.items():
                arrays[f"{name}.{k}"] = np.stack(v)
            zeros = float(np.mean(arrays[f"{name}.raw"] == 0))
            meta["cases"][name] = dict(frames=frames, scene=list(scene), blocks_per_branch=branches,
                                       zero_share=round(zeros, 3),
                                       invalid_share=round(float(np.unpackbits(arrays[f"{name}.invalid_bits"]).mean()), 3))
    meta["numpy"] = np.__version__
    return arrays, meta


def time_full():
    """Seconds of the reference's CPU path for one 256 x 256 x 32 frame: (remap + mask, _downsample_label)."""
    io_data, nyu_preprocess = import_reference()
    lut = io_data.get_remap_lut(YAML)
    rng = np.random.default_rng(7)
    scene = (256, 256, 32)
    raw = synthetic_raw(rng, scene, learning_map_keys())
    invalid = io_data.unpack(synthetic_bits(rng, raw.size, 0.10))
    t0 = time.perf_counter()
    label = lut[raw.astype(np.float32).astype(np.uint16)].astype(np.float32)
    label[np.isclose(invalid, 1)] = 255
    label = label.reshape(scene)
    t1 = time.perf_counter()
    nyu_preprocess._downsample_label(label, scene, 8)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def save(path, arrays, meta):
    arrays = dict(arrays)
    arrays["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(path, **arrays)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "kitti_raw_labels.npz"))
    ap.add_argument("--time-full", action="store_true")
    args = ap.parse_args()
    arrays, meta = generate()
    save(args.out, arrays, meta)
    print(f"wrote {args.out} ({os.path.getsize(args.out) / 1e3:.0f} KB)")
    print(json.dumps(meta["cases"]))
    if args.time_full:
        a, b = time_full()
        print(json.dumps({"reference_cpu_256x256x32": {"remap_mask_ms": round(1e3 * a, 1),
                                                       "downsample_label_ms": round(1e3 * b, 1)}}))
