"""RayIoU of a directory of predicted label volumes against target volumes, without the model
(occdepth_amd/ray_metric.py, K35: the ray-based metric of "Fully Sparse 3D Occupancy Prediction", Liu et al., 2024).

    python tools/ray_metric.py --pred out/sequences/08/predictions --gt .../dataset/sequences/08/voxels
        [--dims 256 256 32] [--origin 0 -25.6 -2] [--voxel-size 0.2] [--classes 20] [--thresholds 1 2 4]
        [--unknown drop|pass] [--origins N [--origin-step 5] --poses .../dataset/sequences/08]
        [--beams 64] [--pitch -24.8 2] [--azimuth -90 90] [--azimuth-step 0.2] [--beam-major] [--every 1]

--pred / --gt name a directory; what it holds decides how it is read (tools/map_sequence.py reads the same):
    <frame>.label                        submission files, the project's own output format (dataset label ids; the inverse
                                         of output.KITTI_LEARNING_MAP_INV brings them back to the 20 training classes, any
                                         other id becomes 255)
    <frame>.label with <frame>.invalid   the dataset's raw voxels, decoded on the GPU (targets.kitti_labels)
    <frame>.pkl                          the pickles of generate_output.py: "y_pred" for --pred, "target" for --gt
The frames both directories hold are scored.  The rays are ray_metric.lidar_directions(...) -- a 64-beam stand-in fan, not
a sensor's calibration table -- cast from the velodyne origin; with --origins N also from the sensor positions of the
frames t, t + step, ... that lie inside the grid (ray_metric.trajectory_origins; --poses is the sequence directory with
poses.txt and calib.txt).  --unknown drop (default): a ray that meets a target voxel 255 before its target hit is left out;
pass: 255 is seen through.  Prints a `ray======` block: RayIoU, RayIoU@tau, the class-agnostic RayIoU_geo, the per-class
table and the ray tallies.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from map_sequence import list_frames, read_frame, submission_inverse_lut  # noqa: E402
from occdepth_amd import fuse, ray_metric  # noqa: E402


def run(args, device=None):
    """-> RayMetrics.get_stats() over the frames --pred and --gt share."""
    device = device or torch.device("cuda")
    dims = tuple(int(d) for d in args.dims)
    if args.origins > 1 and not args.poses:
        raise ValueError("--origins %d needs --poses (the sequence directory with poses.txt and calib.txt)" % args.origins)
    kinds, frames = {}, {}
    for role, src in (("pred", args.pred), ("gt", args.gt)):
        kinds[role], frames[role] = list_frames(src)
    if kinds["pred"] == "raw":
        raise ValueError("%s holds raw dataset voxels: a prediction is <frame>.label (submission) or <frame>.pkl" % args.pred)
    shared = sorted(set(frames["pred"]) & set(frames["gt"]))[::max(int(args.every), 1)]
    if not shared:
        raise FileNotFoundError("%s and %s share no frame" % (args.pred, args.gt))
    dirs = ray_metric.lidar_directions(beams=args.beams, pitch_deg=tuple(args.pitch), azimuth_deg=tuple(args.azimuth),
                                       azimuth_step_deg=args.azimuth_step, tile=None if args.beam_major else 8)
    metric = ray_metric.RayMetrics(args.classes, args.voxel_size, dirs, tuple(args.thresholds), args.unknown)
    poses = fuse.read_kitti_poses(args.poses) if args.origins > 1 else None
    lut = submission_inverse_lut()
    own = ray_metric.sensor_origin(args.origin, args.voxel_size)[None]
    for n in shared:
        pred, _ = read_frame(kinds["pred"], frames["pred"][n], "pred", dims, device, lut=lut)
        gt, _ = read_frame(kinds["gt"], frames["gt"][n], "gt", dims, device, lut=lut)
        origins = own
        if poses is not None:
            if n not in poses:
                raise KeyError("%s has no pose for frame %d" % (args.poses, n))
            origins = ray_metric.trajectory_origins(poses, n, args.origins, args.origin_step, args.origin, args.voxel_size, dims)
        metric.add_batch(pred.reshape((1,) + dims), gt.reshape((1,) + dims), origins[None])
    stats = metric.get_stats()
    print("%d frames, %d rays per origin" % (len(shared), len(dirs)))
    print("\n".join(ray_metric.format_report(stats, [str(c) for c in range(args.classes)], "ray")))
    return stats


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--dims", type=int, nargs=3, default=(256, 256, 32))
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, -25.6, -2.0), help="vox_origin in metres, sensor frame")
    ap.add_argument("--voxel-size", type=float, default=0.2)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--thresholds", type=float, nargs="+", default=(1.0, 2.0, 4.0), help="metres, up to 4")
    ap.add_argument("--unknown", choices=("drop", "pass"), default="drop")
    ap.add_argument("--origins", type=int, default=1)
    ap.add_argument("--origin-step", type=int, default=5)
    ap.add_argument("--poses", default=None)
    ap.add_argument("--beams", type=int, default=64)
    ap.add_argument("--pitch", type=float, nargs=2, default=(-24.8, 2.0))
    ap.add_argument("--azimuth", type=float, nargs=2, default=(-90.0, 90.0))
    ap.add_argument("--azimuth-step", type=float, default=0.2)
    ap.add_argument("--beam-major", action="store_true", help="plain beam-major ray order instead of 8 x 8 tiles")
    ap.add_argument("--every", type=int, default=1)
    return ap


if __name__ == "__main__":
    run(parser().parse_args())
