"""Panoptic quality of a directory of predicted label volumes against target volumes, without the model
(occdepth_amd/panoptic.py, K40: PQ / SQ / RQ of the connected components of the things classes and of the stuff classes, the
components found, numbered and overlapped on the GPU).

    python tools/panoptic.py --pred out/sequences/08/predictions --gt .../dataset/sequences/08/voxels
        [--dims 256 256 32] [--classes 20] [--things 1 2 3 4 5 6 7 8] [--stuff 9 ... 19] [--connectivity 26]
        [--min-voxels 1] [--every 1]

--pred / --gt name a directory; what it holds decides how it is read (tools/map_sequence.py and tools/dist_metric.py read
the same): <frame>.label submission files, <frame>.label with <frame>.invalid raw dataset voxels, or <frame>.pkl pickles
("y_pred" for --pred, "target" for --gt).  The frames both directories hold are scored.  The target's "instances" are the
connected components of the target volume -- the completion volumes carry no instance annotation.  Target voxels 255 do not
count.  --min-voxels N removes the prediction's components of fewer than N voxels first.  Prints a `pan======` block.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_sequence import list_frames, read_frame, submission_inverse_lut  # noqa: E402
from occdepth_amd import panoptic as pan  # noqa: E402


def run(args, device=None):
    """-> PanopticMetrics.get_stats() over the frames --pred and --gt share."""
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
    metric = pan.PanopticMetrics(args.classes, tuple(args.things), tuple(args.stuff), args.connectivity, args.min_voxels)
    lut = submission_inverse_lut()
    for n in shared:
        pred, _ = read_frame(kinds["pred"], frames["pred"][n], "pred", dims, device, lut=lut)
        gt, _ = read_frame(kinds["gt"], frames["gt"][n], "gt", dims, device, lut=lut)
        metric.add_batch(pred.reshape((1,) + dims), gt.reshape((1,) + dims))
    stats = metric.get_stats()
    print("%d frames" % len(shared))
    print("\n".join(pan.format_report(stats, [str(c) for c in range(args.classes)], "pan")))
    return stats


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--dims", type=int, nargs=3, default=(256, 256, 32))
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--things", type=int, nargs="*", default=pan.KITTI_THINGS)
    ap.add_argument("--stuff", type=int, nargs="*", default=pan.KITTI_STUFF)
    ap.add_argument("--connectivity", type=int, default=26, choices=(6, 26))
    ap.add_argument("--min-voxels", type=int, default=1, help="remove the prediction's components of fewer voxels first")
    ap.add_argument("--every", type=int, default=1)
    return ap


if __name__ == "__main__":
    run(parser().parse_args())
