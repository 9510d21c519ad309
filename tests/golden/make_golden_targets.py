"""Generate tests/golden/train_targets.npz: the reference's OWN dataloader target functions on CPU.

    python tests/golden/make_golden_targets.py [--out PATH]

Runs where the reference checkout exists (not on the GPU machines).  It imports the real
  compute_local_frustums, compute_CP_mega_matrix   occdepth/data/utils/helpers.py:6-91,183-260
  _downsample_label                                occdepth/data/NYU/preprocess.py:102-143
with `hydra`, `omegaconf` and `occdepth.data.utils.fusion` stubbed in sys.modules (the three functions use none of
them); the voxel -> pixel tables come from oracle.inputs.vox2pix (pinned bit for bit to the GPU projection).

Two cases:
  full   256 x 256 x 32, stereo KITTI calibration (inputs.KITTI_TR / KITTI_K, right view 0.54 m to the side), 1220 x 370,
         frustum_size 8, a structured target whose 8^3 blocks hit every branch of _downsample_label.  The masks are stored
         as per-frustum digests (count, index sum, CRC32 of np.packbits) -- 134 MB of bits do not fit a fixture --
         for both views and for the left view alone; the dists in full; target_1_8; both CP matrices as packbits.
  small  the kitti_small geometry (64 x 64 x 16, 320 x 96): target of golden_cases.train_extras("kitti_small", ...),
         calibration of golden_cases.occdepth_batch("kitti_small"); masks as packbits.
  mixed  the small target with every third 8^3 block emptied (mixed_target), stereo only: the training-step tests.
Only inputs the tests rebuild and the reference's outputs are stored.
"""
import argparse
import json
import os
import sys
import time
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import inputs  # noqa: E402
from oracle.ref_shims import REF_ROOT  # noqa: E402

FULL = dict(scene=(256, 256, 32), img_wh=(1220, 370), frustum_size=8, n_classes=20)
SMALL = dict(scene=(64, 64, 16), img_wh=(320, 96), frustum_size=8, n_classes=20)
VOXEL = 0.2


def import_reference():
    sys.path.insert(0, REF_ROOT)
    for name in ("hydra", "omegaconf", "occdepth.data.utils.fusion"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["hydra"].main = lambda *a, **k: (lambda f: f)
    sys.modules["omegaconf"].DictConfig = dict
    import occdepth.data.utils.helpers as helpers
    import occdepth.data.NYU.preprocess as preprocess
    return helpers, preprocess


def calibration(scale_k=1.0):
    """(cam_E (2, 4, 4), cam_k (2, 3, 3)) float64: inputs.kitti_batch's stereo pair."""
    k = inputs.KITTI_K.copy()
    k[:2] *= scale_k
    tr2 = inputs.KITTI_TR.copy()
    tr2[0, 3] = -0.54
    return np.stack([inputs.KITTI_TR, tr2]), np.stack([k, k])


def origin(scene):
    return (0.0, -0.1 * scene[1], -2.0)          # kitti_dataset.py:82 for the full scene; centred in y for reduced ones


def structured_target(scene=(256, 256, 32)):
    """Boxes of labels, large empty and unlabelled regions, and crafted 8^3 blocks for every _downsample_label branch."""
    rng = np.random.default_rng(20260)
    t = np.zeros(scene, dtype=np.uint8)
    X, Y, Z = scene
    for _ in range(60):                                            # random boxes of labels 1..19
        x0, y0, z0 = rng.integers(0, X - 8), rng.integers(0, Y - 8), rng.integers(0, Z - 4)
        dx, dy, dz = rng.integers(4, 40), rng.integers(4, 40), rng.integers(2, 12)
        t[x0:x0 + dx, y0:y0 + dy, z0:z0 + dz] = rng.integers(1, 20)
    t[:, 200:, :] = 255                                            # a large unlabelled region (outside the "FOV")
    t[180:256, 0:40, 20:32] = 255
    speck = rng.random(scene) < 0.03                               # scattered labels and holes everywhere
    t[speck] = rng.integers(0, 20, size=int(speck.sum()), dtype=np.uint8)
    t[rng.random(scene) < 0.02] = 255

    def block(bx, by, bz, values):
        v = np.asarray(values, dtype=np.uint8)
        assert v.size == 512
        t[8 * bx:8 * bx + 8, 8 * by:8 * by + 8, 8 * bz:8 * bz + 8] = rng.permutation(v).reshape(8, 8, 8)

    def fill(*pairs):
        out = []
        for lab, n in pairs:
            out += [lab] * n
        assert len(out) == 512, len(out)
        return out

    crafted = [
        fill((0, 512)),                              # all empty -> 0
        fill((255, 512)),                            # all unlabelled -> 255
        fill((0, 256), (255, 256)),                  # #0 == #255 above the threshold -> 255 (tie)
        fill((0, 257), (255, 255)),                  # #0 > #255 -> 0
        fill((0, 255), (255, 257)),                  # #0 < #255 -> 255
        fill((0, 487), (5, 25)),                     # 487 > 486.4 -> 0
        fill((0, 200), (255, 286), (7, 26)),         # 486 -> argmax of the labels: 7
        fill((0, 486), (3, 13), (9, 13)),            # argmax tie 3 / 9 -> 3 (smallest)
        fill((12, 100), (4, 100), (0, 312)),         # argmax tie 4 / 12 -> 4
        fill((19, 10), (2, 9), (0, 493)),            # 493 empty -> 0 although labels present
        fill((1, 170), (2, 171), (3, 171)),          # no empty: argmax 2 / 3 tie -> 2
        fill((17, 512)),                             # a full block of one class
        fill((255, 300), (6, 20), (8, 20), (0, 172)),  # below the threshold (472): argmax tie 6 / 8 -> 6
    ]
    for i, vals in enumerate(crafted):
        block(2 + i, 10 + (i % 3), i % 4, vals)
    return t


def frustum_digests(masks):
    """(F, X, Y, Z) bool -> (F, 3) int64: voxel count, sum of flat indices, CRC32 of np.packbits of the flat plane."""
    out = np.zeros((masks.shape[0], 3), dtype=np.int64)
    for f in range(masks.shape[0]):
        flat = masks[f].reshape(-1)
        idx = np.flatnonzero(flat)
        out[f] = (idx.size, int(idx.sum()), zlib.crc32(np.packbits(flat).tobytes()))
    return out


def reference_frustums(helpers, target, cam_E, cam_k, scene, img_wh, frustum_size, n_classes, views):
    pix, z = [], []
    for v in views:
        p, _, pz = inputs.vox2pix(cam_E[v], cam_k[v], origin(scene), VOXEL, img_wh[0], img_wh[1],
                                  tuple(s * VOXEL for s in scene), 0)
        pix.append(p)
        z.append(pz)
    pix = np.stack(pix)                                            # (V, N, 1, 2), as kitti_dataset.py:276-283 stacks it
    assert pix.shape == (len(views), int(np.prod(scene)), 1, 2), pix.shape
    masks, dists = helpers.compute_local_frustums(pix, np.stack(z), target, img_wh[0], img_wh[1], dataset="kitti",
                                                  n_classes=n_classes, size=frustum_size)
    return masks, dists


def small_target():
    import golden_cases as gc
    ex = gc.train_extras("kitti_small", {}, SMALL["scene"], SMALL["n_classes"], (96, 320))
    return ex["target"][0].numpy().astype(np.uint8)


def mixed_target(t):
    """The kitti_small target with every third 8^3 block emptied: its 1:8 labels then hold 0 next to classes, so all
    four relation planes have positives (the seeded target alone gives none to the two "empty" planes)."""
    t = t.copy()
    for xs in range(t.shape[0] // 8):
        for ys in range(t.shape[1] // 8):
            for zs in range(t.shape[2] // 8):
                if (xs + ys + zs) % 3 == 0:
                    t[8 * xs:8 * xs + 8, 8 * ys:8 * ys + 8, 8 * zs:8 * zs + 8] = 0
    return t


def generate():
    helpers, preprocess = import_reference()
    arrays, meta = {}, {}
    t0 = time.time()
    # ---------------------------------------------------------------- full size
    tgt = structured_target(FULL["scene"])
    E, K = calibration(1.0)
    arrays["full.cam_E"], arrays["full.cam_k"] = E, K
    for tag, views in (("stereo", [0, 1]), ("left", [0])):
        masks, dists = reference_frustums(helpers, tgt, E, K, FULL["scene"], FULL["img_wh"], FULL["frustum_size"],
                                          FULL["n_classes"], views)
        arrays[f"full.{tag}.mask_digest"] = frustum_digests(masks)
        arrays[f"full.{tag}.dists"] = dists.astype(np.float64)
    t18 = preprocess._downsample_label(tgt, FULL["scene"], 8)
    arrays["full.target_1_8"] = t18
    for tag, binary in (("cp4", False), ("cp2", True)):
        cp = helpers.compute_CP_mega_matrix(t18, is_binary=binary)
        arrays[f"full.{tag}.shape"] = np.asarray(cp.shape, dtype=np.int64)
        arrays[f"full.{tag}.bits"] = np.packbits(cp.reshape(-1))
    arrays["full.target"] = tgt
    # ---------------------------------------------------------------- kitti_small
    tgt_s = small_target()
    Es, Ks = calibration(320 / 1220)
    arrays["small.cam_E"], arrays["small.cam_k"] = Es, Ks
    arrays["small.target"] = tgt_s
    for tag, views in (("stereo", [0, 1]), ("left", [0])):
        masks, dists = reference_frustums(helpers, tgt_s, Es, Ks, SMALL["scene"], SMALL["img_wh"], SMALL["frustum_size"],
                                          SMALL["n_classes"], views)
        arrays[f"small.{tag}.mask_shape"] = np.asarray(masks.shape, dtype=np.int64)
        arrays[f"small.{tag}.mask_bits"] = np.packbits(masks.reshape(-1))
        arrays[f"small.{tag}.dists"] = dists.astype(np.float64)
    t18s = preprocess._downsample_label(tgt_s, SMALL["scene"], 8)
    arrays["small.target_1_8"] = t18s
    for tag, binary in (("cp4", False), ("cp2", True)):
        cp = helpers.compute_CP_mega_matrix(t18s, is_binary=binary)
        arrays[f"small.{tag}.shape"] = np.asarray(cp.shape, dtype=np.int64)
        arrays[f"small.{tag}.bits"] = np.packbits(cp.reshape(-1))
    # ---------------------------------------------------------------- kitti_small, mixed 1:8 labels (training-step tests)
    tgt_m = mixed_target(tgt_s)
    arrays["mixed.target"] = tgt_m
    masks, dists = reference_frustums(helpers, tgt_m, Es, Ks, SMALL["scene"], SMALL["img_wh"], SMALL["frustum_size"],
                                      SMALL["n_classes"], [0, 1])
    arrays["mixed.stereo.mask_shape"] = np.asarray(masks.shape, dtype=np.int64)
    arrays["mixed.stereo.mask_bits"] = np.packbits(masks.reshape(-1))
    arrays["mixed.stereo.dists"] = dists.astype(np.float64)
    t18m = preprocess._downsample_label(tgt_m, SMALL["scene"], 8)
    arrays["mixed.target_1_8"] = t18m
    cp = helpers.compute_CP_mega_matrix(t18m)
    arrays["mixed.cp4.shape"] = np.asarray(cp.shape, dtype=np.int64)
    arrays["mixed.cp4.bits"] = np.packbits(cp.reshape(-1))
    meta.update(full=dict(FULL, origin=origin(FULL["scene"]), voxel=VOXEL),
                small=dict(SMALL, origin=origin(SMALL["scene"]), voxel=VOXEL), numpy=np.__version__,
                seconds=round(time.time() - t0, 1))
    return arrays, meta


def save(path, arrays, meta):
    arrays = dict(arrays)
    arrays["__meta__"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(path, **arrays)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "train_targets.npz"))
    args = ap.parse_args()
    arrays, meta = generate()
    save(args.out, arrays, meta)
    print(f"wrote {args.out} ({os.path.getsize(args.out) / 1e6:.2f} MB) in {meta['seconds']} s")
