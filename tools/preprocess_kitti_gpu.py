"""The reference's SemanticKITTI label preprocessing (occdepth/data/semantic_kitti/preprocess.py) on the GPU.

    python tools/preprocess_kitti_gpu.py <data_root> <out_root> [--sequences 00 01 ...] [--batch 8]

Reads  <data_root>/dataset/sequences/<seq>/voxels/<frame>.label and .invalid   (preprocess.py:58-66)
writes <out_root>/labels/<seq>/<frame>_1_1.npy   float32 (256, 256, 32): remapped labels, 255 where invalid
       <out_root>/labels/<seq>/<frame>_1_8.npy   uint8   (32, 32, 4):    _downsample_label of the above
with targets.kitti_labels(check=True) and targets.downsample_label, several frames per launch.  A file that exists is
left alone, as the reference does (preprocess.py:90).  Training does not need these files: a batch that carries the raw
voxel files is decoded inside the step; this tool is for whoever wants the reference's `labels/` tree.
"""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import targets  # noqa: E402

SEQUENCES = ("00", "01", "02", "03", "04", "05", "06", "07", "08", "09", "10")
SCENE_SIZE = (256, 256, 32)


def preprocess_sequence(voxel_dir, out_dir, scene_size=SCENE_SIZE, batch=8, device="cuda"):
    """Every `<frame>.label` of `voxel_dir` -> `<out_dir>/<frame>_1_1.npy` and `_1_8.npy`; returns the paths written (none
    for frames whose two files already exist -- those are not even read)."""
    os.makedirs(out_dir, exist_ok=True)
    todo = []
    for path in sorted(glob.glob(os.path.join(voxel_dir, "*.label"))):
        frame = os.path.splitext(os.path.basename(path))[0]
        missing = [s for s in ("1_1", "1_8") if not os.path.exists(os.path.join(out_dir, f"{frame}_{s}.npy"))]
        if missing:
            todo.append((frame, missing))
    written = []
    for i in range(0, len(todo), max(int(batch), 1)):
        chunk = todo[i:i + max(int(batch), 1)]
        files = [targets.read_raw_kitti_voxels(voxel_dir, frame) for frame, _ in chunk]
        raw = torch.from_numpy(np.stack([f[0] for f in files])).to(device)
        invalid = torch.from_numpy(np.stack([f[1] for f in files])).to(device)
        full = targets.kitti_labels(raw, invalid, scene_size=scene_size, check=True)
        coarse = targets.downsample_label(full, 8).cpu().numpy()
        full = full.cpu().numpy()
        for j, (frame, missing) in enumerate(chunk):
            for scale, vol in (("1_1", full[j].astype(np.float32)), ("1_8", coarse[j])):
                if scale in missing:
                    path = os.path.join(out_dir, f"{frame}_{scale}.npy")
                    np.save(path, vol)
                    written.append(path)
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("data_root")
    ap.add_argument("out_root")
    ap.add_argument("--sequences", nargs="*", default=list(SEQUENCES))
    ap.add_argument("--batch", type=int, default=8, help="frames per launch")
    args = ap.parse_args()
    for seq in args.sequences:
        voxel_dir = os.path.join(args.data_root, "dataset", "sequences", seq, "voxels")
        written = preprocess_sequence(voxel_dir, os.path.join(args.out_root, "labels", seq), batch=args.batch)
        print(f"sequence {seq}: wrote {len(written)} files")


if __name__ == "__main__":
    main()
