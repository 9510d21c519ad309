"""Stereo depth maps for a rectified image pair -- or two directories of pairs -- matched on the GPU (occdepth_amd/stereo.py)
and written as 16-bit PNGs of round(depth * 256), 0 = no measurement, clipped to 65535: the files the reference's
`load_depth` reads (kitti_dataset.py:40-44), so its unmodified loader can consume them in place of the side dataset.

    python tools/stereo_depth.py image_2/000000.png image_3/000000.png --focal 707.0912 --baseline 0.54 -o depth/000000.png
    python tools/stereo_depth.py sequences/00/image_2 sequences/00/image_3 --focal 707.0912 --baseline 0.54 -o depth/00

Two directories: every file name present in both is matched and written under the output directory.  --max-disp is a
multiple of 64 in 64..256 (192 reaches 2 m at KITTI's f B of 382 px m)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import stereo  # noqa: E402


def read_gray(path):
    """An image file -> (H, W) uint8 with the matcher's own gray formula."""
    from PIL import Image
    rgb = np.asarray(Image.open(path).convert("RGB")).astype(np.int32)
    return ((77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8).astype(np.uint8)


def depth_png(left, right, focal, baseline, max_disp=stereo.MAX_DISP, device="cuda"):
    """gray left / right (H, W) uint8 -> (H, W) uint16 PNG values."""
    if left.shape != right.shape:
        raise ValueError("the two images differ in size: %s and %s" % (left.shape, right.shape))
    pair = torch.from_numpy(np.stack([left, right]))[None].to(device)
    disp = stereo.sgm_disparity(pair, max_disp)[0].cpu().numpy()
    fB = np.float32(np.float64(focal) * np.float64(baseline))
    with np.errstate(divide="ignore"):
        depth = np.where(disp > 0, fB / disp, np.float32(0)).astype(np.float32)
    return stereo.depth_to_png16(depth)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("left")
    ap.add_argument("right")
    ap.add_argument("--focal", type=float, required=True, help="focal length of the left camera in pixels")
    ap.add_argument("--baseline", type=float, required=True, help="distance between the two cameras in metres")
    ap.add_argument("--max-disp", type=int, default=stereo.MAX_DISP)
    ap.add_argument("-o", "--out", required=True, help="output PNG, or output directory for two input directories")
    args = ap.parse_args()
    if os.path.isdir(args.left) != os.path.isdir(args.right):
        ap.error("left and right must both be files or both be directories")
    if os.path.isdir(args.left):
        names = sorted(set(os.listdir(args.left)) & set(os.listdir(args.right)))
        if not names:
            ap.error("no file name is present in both directories")
        os.makedirs(args.out, exist_ok=True)
        jobs = [(os.path.join(args.left, n), os.path.join(args.right, n),
                 os.path.join(args.out, os.path.splitext(n)[0] + ".png")) for n in names]
    else:
        jobs = [(args.left, args.right, args.out)]
    for left, right, out in jobs:
        png = depth_png(read_gray(left), read_gray(right), args.focal, args.baseline, args.max_disp)
        stereo.write_png16(out, png)
        print("%s: %.1f %% of the pixels measured" % (out, 100.0 * float((png > 0).mean())))


if __name__ == "__main__":
    main()
