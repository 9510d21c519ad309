"""Distance-tolerant scores of a directory of predicted label volumes against target volumes, without the model
(occdepth_amd/dist_metric.py, K37: precision / recall / F-score at a distance and the Chamfer distance between occupied
voxels, class-agnostic and per class, from the exact distance transform on the GPU).

    python tools/dist_metric.py --pred out/sequences/08/predictions --gt .../dataset/sequences/08/voxels
        [--dims 256 256 32] [--voxel-size 0.2] [--classes 20] [--thresholds 0.2 0.4 0.8] [--max-d2 1024] [--every 1]

--pred / --gt name a directory; what it holds decides how it is read (tools/map_sequence.py reads the same):
    <frame>.label                        submission files, the project's own output format (dataset label ids; the inverse
                                         of output.KITTI_LEARNING_MAP_INV brings them back to the 20 training classes, any
                                         other id becomes 255)
    <frame>.label with <frame>.invalid   the dataset's raw voxels, decoded on the GPU (targets.kitti_labels)
    <frame>.pkl                          the pickles of generate_output.py: "y_pred" for --pred, "target" for --gt
The frames both directories hold are scored.  Target voxels 255 are no queries.  Prints a `dist======` block: F, precision
and recall of the occupied voxels and the mean F over the classes per threshold, the Chamfer distances (truncated at
voxel_size * sqrt(max_d2 + 1) per side) and the per-class table.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_sequence import list_frames, read_frame, submission_inverse_lut  # noqa: E402
from occdepth_amd import dist_metric  # noqa: E402


def run(args, device=None):
    """-> DistanceMetrics.get_stats() over the frames --pred and --gt share."""
    device = device or torch.device("cuda")
    dims = tuple(int(d) for d in args.dims)
    kinds, frames = {}, {}
    for role, src in (("pred", args.pred), ("gt", args.gt)):
        kinds[role], frames[role] = list_frames(src)
    if kinds["pred"] == "raw":
        raise ValueError("%s holds raw dataset voxels: a prediction is <frame>.label (submission) or <frame>.pkl" % args.pred)
    shared = sorted(set(frames["pred"]) & set(frames["gt"]))[::max(int(args.every), 1)]
    if not shared:
        raise FileNotFoundError("%s and %s share no frame" % (args.pred, args.gt))
    metric = dist_metric.DistanceMetrics(args.classes, args.voxel_size, tuple(args.thresholds), args.max_d2)
    lut = submission_inverse_lut()
    for n in shared:
        pred, _ = read_frame(kinds["pred"], frames["pred"][n], "pred", dims, device, lut=lut)
        gt, _ = read_frame(kinds["gt"], frames["gt"][n], "gt", dims, device, lut=lut)
        metric.add_batch(pred.reshape((1,) + dims), gt.reshape((1,) + dims))
    stats = metric.get_stats()
    print("%d frames" % len(shared))
    print("\n".join(dist_metric.format_report(stats, [str(c) for c in range(args.classes)], "dist")))
    return stats


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--dims", type=int, nargs=3, default=(256, 256, 32))
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--thresholds", type=float, nargs="+", default=(0.2, 0.4, 0.8), help="metres")
    ap.add_argument("--max-d2", type=int, default=1024, help="truncation of the squared voxel distance")
    ap.add_argument("--every", type=int, default=1)
    return ap


if __name__ == "__main__":
    run(parser().parse_args())
