"""Build the semantic map of one sequence offline (occdepth_amd/semantic_map.py) from per-frame label volumes, write it
as a point PLY, and score a prediction map against a ground-truth map.

    python tools/map_sequence.py --poses .../dataset/sequences/08 --pred out/08 --gt .../dataset/sequences/08/voxels \\
        --out maps/08 [--min-obs 2] [--fov] [--every 5] [--views bev oblique] [--png-side 2048] [--camera-every 50 --t-max 80]
        [--frames-out DIR [--exclude-self] [--keep-own]] [--frame-range FIRST LAST] [--save-map PREFIX] [--load-map PREFIX ...]
        [--visibility W_VIS W_HID] [--mesh [--mesh-open]]

--pred / --gt name a directory; what it holds decides how it is read:
    <frame>.pkl                          the pickles of generate_output.py (occdepth_amd.output.write_outputs): "y_pred"
                                         for --pred, "target" for --gt; with --fov the frame votes inside its "fov_mask_1"
    <frame>.label                        submission files (dataset label ids, the inverse of output.KITTI_LEARNING_MAP_INV
                                         brings them back to the 20 training classes; any other id does not vote)
    <frame>.label with <frame>.invalid   the dataset's raw voxels, decoded on the GPU (targets.kitti_labels)
--poses is the sequence directory with poses.txt and calib.txt.  Writes <out>_pred.ply / <out>_gt.ply and, given both
sources, prints the map's Precision / Recall / IoU / mIoU over the voxels both maps observed.  --views also draws the maps
(render.render_map, the bricks ray-cast on the GPU) to <out>_{pred,gt,err}_{view}.png; --camera-every N draws them through
the left colour camera (P2 and Tr of calib.txt) of every N-th posed frame to <out>_{pred,gt,err}_camera_<frame>.png.
--frames-out DIR reads the finished prediction map back into every --pred frame (SemanticMap.sample, K32: own = the
frame's labels, inside its mask with --fov; --exclude-self takes the frame's own vote out, --keep-own lets a tie go to the
frame's label) and writes DIR/sequences/<sequence>/predictions/<frame>.label, submission files (<sequence> is the name of
the --poses directory).  When --gt holds per-frame targets it also prints a `frames======` block (the frames' own labels
against their targets) and a `mapped======` block (the sampled labels against the same targets).
--save-map PREFIX keeps the finished maps as PREFIX_pred.occmap / PREFIX_gt.occmap (SemanticMap.save: the vote counters, which
can be voted into again, unlike the PLY); --load-map PREFIX [PREFIX ...] merges such files in (SemanticMap.load, then merge,
K33) before the frames are integrated, and --frame-range FIRST LAST (inclusive) keeps a run to a part of the sequence: one
run over frames 0..1999 with --save-map and a second over 2000..4070 with --load-map give the map of the whole drive.
--visibility W_VIS W_HID makes the prediction map's votes occlusion-aware (occdepth_amd/visibility.py, K34): the pixel rays of
the left colour camera (P2 and Tr of calib.txt, --camera-size) are cast through every --pred frame's own labels; a voxel a ray
reaches, up to and including the first occupied one, votes with W_VIS, any other (inside the mask with --fov) with W_HID.  The
ground-truth map votes as before; --frames-out hands each frame's weights back to the read-back.
--mesh also writes the maps' surfaces, <out>_pred_mesh.ply / <out>_gt_mesh.ply (occdepth_amd/mesh.py, K39): one quad per exposed
voxel face, every lattice corner once, closed towards unobserved space; --mesh-open keeps only the faces towards observed free space.
"""
import argparse
import glob
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import fuse, output, render, semantic_map as sm, targets  # noqa: E402


def submission_inverse_lut():
    """dataset label id -> training class, 255 for an id the submission format never writes."""
    lut = np.full(1 << 16, 255, dtype=np.uint8)
    for train_id, label_id in enumerate(output.KITTI_LEARNING_MAP_INV):
        lut[label_id] = train_id
    return lut


def list_frames(src):
    """-> (kind, {frame index: path without extension}); kind is "pkl", "raw" or "label"."""
    for kind, pattern in (("pkl", "*.pkl"), ("label", "*.label")):
        paths = sorted(glob.glob(os.path.join(src, pattern)))
        if paths:
            frames = {int(os.path.splitext(os.path.basename(p))[0]): os.path.splitext(p)[0] for p in paths}
            if kind == "label" and all(os.path.exists(b + ".invalid") for b in frames.values()):
                kind = "raw"
            return kind, frames
    raise FileNotFoundError("%s holds neither <frame>.pkl nor <frame>.label files" % src)


def read_frame(kind, base, role, dims, device, use_fov=False, lut=None):
    """-> (labels (X, Y, Z) uint8 on `device`, mask or None)."""
    if kind == "pkl":
        with open(base + ".pkl", "rb") as f:
            d = pickle.load(f)
        key = "y_pred" if role == "pred" else "target"
        if key not in d:
            raise KeyError("%s.pkl has no %r" % (base, key))
        lab = np.asarray(d[key]).astype(np.uint16)
        lab = np.where(lab > 255, 255, lab).astype(np.uint8).reshape(dims)
        mask = None
        if use_fov:
            mask = torch.from_numpy(np.asarray(d["fov_mask_1"]).reshape(-1)[:lab.size] != 0).to(device)
        return torch.from_numpy(lab).to(device), mask
    if kind == "label":
        raw = np.fromfile(base + ".label", dtype=np.uint16)
        return torch.from_numpy(lut[raw].reshape(dims)).to(device), None
    raw, invalid = targets.read_raw_kitti_voxels(os.path.dirname(base), os.path.basename(base))
    lab = targets.kitti_labels(torch.from_numpy(raw.view(np.int16))[None].to(device), torch.from_numpy(invalid)[None].to(device),
                               scene_size=dims)
    return lab[0], None


def visibility_weight(labels, mask, args):
    """--visibility: the vote weights of one prediction frame from its own labels -- the pixel rays of the left colour
    camera (calib.txt, --camera-size) carve the volume (occdepth_amd.visibility, K34) -- or None without the switch."""
    if not args.visibility:
        return None
    from occdepth_amd import visibility
    if getattr(args, "_rays", None) is None:                               # one view for the whole sequence
        cam_k, E = read_camera(args.poses)
        args._rays = visibility.camera_rays(torch.from_numpy(cam_k), torch.from_numpy(E), tuple(args.origin), args.voxel,
                                            tuple(args.camera_size))
    view, size = args._rays
    return visibility.vote_weights(visibility.visible_voxels(labels, view, size), mask, *args.visibility)


def build_map(src, role, poses, args, device):
    kind, frames = list_frames(src)
    lut = submission_inverse_lut() if kind == "label" else None
    m = sm.SemanticMap(args.classes, args.voxel, args.origin, tuple(args.dims), max_bricks=args.max_bricks)
    for prefix in args.load_map or ():                                     # votes commute: earlier runs' maps come first or last alike
        path = "%s_%s.occmap" % (prefix, role)
        m.merge(sm.SemanticMap.load(path, device=device))
        print("%s: merged %s -> %d bricks" % (role, path, m.n_bricks))
    used = 0
    first, last = args.frame_range if args.frame_range else (min(frames), max(frames))
    for frame in [f for f in sorted(frames) if first <= f <= last][::args.every]:
        if frame not in poses:
            raise KeyError("no pose for frame %d of %s (%s)" % (frame, src, os.path.join(args.poses, "poses.txt")))
        labels, mask = read_frame(kind, frames[frame], role, tuple(args.dims), device, args.fov, lut)
        if role == "pred" and int(getattr(args, "min_component", 0) or 0) > 1:      # speckle does not vote
            from occdepth_amd import panoptic
            labels = panoptic.remove_small_components(labels.contiguous(), args.min_component, panoptic.KITTI_THINGS)
        weight = visibility_weight(labels, mask, args) if role == "pred" else None
        if weight is not None:
            m.integrate(labels, poses[frame], weight=weight)
        else:
            m.integrate(labels, poses[frame], mask=mask)
        used += 1
    print("%s: %d %s frames of %s -> %d bricks, %.1f MB" % (role, used, kind, src, m.n_bricks, m.n_bricks * m.brick_bytes / 1e6))
    return m


def _print_block(name, stats, classes):
    print("%s======" % name)
    print("Precision={:.4f}, Recall={:.4f}, IoU={:.4f}".format(stats["precision"] * 100, stats["recall"] * 100, stats["iou"] * 100))
    print(" ".join(["{:.4f}, "] * classes).format(*(stats["iou_ssc"] * 100).tolist()))
    print("mIoU={:.4f}".format(stats["iou_ssc_mean"] * 100))


def sample_frames(pred_map, poses, args, device):
    """--frames-out: every --pred frame sampled back from the finished prediction map and written as a submission file;
    with per-frame targets in --gt also scored -> (paths, {"frames": stats, "mapped": stats} or None)."""
    from occdepth_amd.loss.sscMetrics import SSCMetrics
    dims = tuple(args.dims)
    kind, frames = list_frames(args.pred)
    lut = submission_inverse_lut() if kind == "label" else None
    gt_kind, gt_frames = list_frames(args.gt) if args.gt else (None, {})
    gt_lut = submission_inverse_lut() if gt_kind == "label" else None
    metrics = {"frames": SSCMetrics(args.classes), "mapped": SSCMetrics(args.classes)} if gt_frames else None
    sequence = os.path.basename(os.path.normpath(args.poses))
    paths, scored = [], 0
    for frame in sorted(frames)[::args.every]:
        own, mask = read_frame(kind, frames[frame], "pred", dims, device, args.fov, lut)
        weight = visibility_weight(own, mask, args)                        # what the frame voted with, made again
        voted = {"own_mask": mask} if weight is None else {"own_weight": weight}
        mapped, _ = pred_map.sample(poses[frame], own=own, min_obs=args.min_obs, exclude_self=args.exclude_self,
                                    keep_own=args.keep_own, **voted)
        paths.append(output.write_kitti_submission_labels(mapped, sequence, "%06d" % frame, args.frames_out))
        if frame in gt_frames:
            target, _ = read_frame(gt_kind, gt_frames[frame], "gt", dims, device, False, gt_lut)
            for name, labels in (("frames", own), ("mapped", mapped)):          # a voxel without a label or a target is not counted
                void = (labels >= args.classes) | (target >= args.classes)
                metrics[name].add_batch(labels[None], torch.where(void, torch.full_like(target, 255), target)[None])
            scored += 1
    print("%d frames sampled from the prediction map -> %s" % (len(paths), os.path.join(args.frames_out, "sequences", sequence, "predictions")))
    if not scored:
        return paths, None
    stats = {name: m.get_stats() for name, m in metrics.items()}
    for name in ("frames", "mapped"):
        _print_block(name, stats[name], args.classes)
    return paths, stats


def read_camera(seq_dir):
    """calib.txt -> (cam_k (3, 3), sensor -> left colour camera (4, 4)), float64: cam_k = P2[:, :3] and the extrinsic is
    Tr shifted by K^-1 P2[:, 3] (P2 projects from the rectified camera 0 frame, which Tr maps the sensor into)."""
    rows = {}
    with open(os.path.join(seq_dir, "calib.txt")) as f:
        for line in f:
            name, _, rest = line.partition(":")
            if rest.strip():
                rows[name.strip()] = np.array([float(x) for x in rest.split()], dtype=np.float64)
    missing = [k for k in ("P2", "Tr") if k not in rows or rows[k].size != 12]
    if missing:
        raise KeyError("%s has no %s row of 12 numbers" % (os.path.join(seq_dir, "calib.txt"), " / ".join(missing)))
    P2 = rows["P2"].reshape(3, 4)
    E = np.eye(4)
    E[:3] = rows["Tr"].reshape(3, 4)
    E[:3, 3] += np.linalg.solve(P2[:, :3], P2[:, 3])
    return P2[:, :3].copy(), E


def draw(maps, poses, args, colours):
    """The pictures of --views and --camera-every, next to the PLYs -> the paths."""
    pred = maps.get("pred") or maps["gt"]
    volume = sm.MapVolume(pred, maps.get("gt") if "pred" in maps else None, args.min_obs)
    paths = []
    if args.views:
        if "pred" in maps:
            paths += render.write_map_pictures(volume, args.out, args.views, bev_side=args.png_side, palette=colours)
        else:                                                              # a ground-truth map alone
            views, sizes = render.map_standard_views(args.views, volume, args.png_side)
            for name, img in zip(args.views, render.render_map(volume, views, sizes, palette=colours)):
                paths.append(render.write_png("%s_gt_%s.png" % (args.out, name), img))
    if args.camera_every:
        cam_k, E = read_camera(args.poses)
        size = tuple(args.camera_size)
        kinds = [("pred" if "pred" in maps else "gt", volume, "class")]
        if volume.target is not None:
            kinds += [("gt", volume.target_volume(), "class"), ("err", volume, "error")]
        for frame in sorted(poses)[::args.camera_every]:
            view = render.map_camera_view(cam_k, E, poses[frame], volume)
            for kind, vol, mode in kinds:
                img = render.render_map(vol, view, size, mode=mode, palette=colours, t_max=args.t_max)[0]
                paths.append(render.write_png("%s_%s_camera_%06d.png" % (args.out, kind, frame), img))
    print("%d pictures, window %d x %d x %d voxels, %d bricks" % ((len(paths),) + volume.dims + (volume.n_rows,)))
    return paths


def write_meshes(maps, args, colours):
    """--mesh: <out>_pred_mesh.ply / <out>_gt_mesh.ply, the surfaces of the maps (occdepth_amd.mesh, K39) -> the paths."""
    from occdepth_amd import mesh
    closed = not args.mesh_open
    if "pred" in maps and "gt" in maps:
        parts = dict(zip(("pred", "gt"), mesh.mesh_map(maps["pred"], maps["gt"], args.min_obs, cap_unknown=closed)))
    else:
        role = "pred" if "pred" in maps else "gt"
        parts = {role: mesh.mesh_map(maps[role], None, args.min_obs, cap_unknown=closed)}
    paths = []
    for role, part in parts.items():
        paths.append(mesh.write_mesh_ply("%s_%s_mesh.ply" % (args.out, role), part, colours))
        print("%s: %d faces, %d vertices (%s surface)" % (paths[-1], part.n_faces, part.n_vertices, "closed" if closed else "open"))
    return paths


def run(args, device=None):
    device = device or torch.device("cuda")
    poses = fuse.read_kitti_poses(args.poses)
    colours = render.palette("kitti" if args.classes == 20 else args.classes)
    maps = {}
    for role in ("pred", "gt"):
        src = getattr(args, role)
        if src:
            m = maps[role] = build_map(src, role, poses, args, device)
            coords, labels, n_obs = m.extract(min_obs=args.min_obs)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            path = sm.write_ply("%s_%s.ply" % (args.out, role), coords, labels, n_obs, m.voxel_size, colours)
            print("%s: %d voxels with at least %d vote(s)" % (path, len(labels), args.min_obs))
            if args.save_map:
                os.makedirs(os.path.dirname(os.path.abspath(args.save_map)), exist_ok=True)
                print("%s: the vote counters" % m.save("%s_%s.occmap" % (args.save_map, role)))
    if not maps:
        raise SystemExit("give --pred, --gt or both")
    if args.views or args.camera_every:
        draw(maps, poses, args, colours)
    if args.mesh:
        write_meshes(maps, args, colours)
    stats = None
    if len(maps) == 2:
        from occdepth_amd.loss.sscMetrics import SSCMetrics
        stats = sm.map_confusion(maps["pred"], maps["gt"], SSCMetrics(args.classes)).get_stats()
        print("map======")
        print("Precision={:.4f}, Recall={:.4f}, IoU={:.4f}".format(stats["precision"] * 100, stats["recall"] * 100, stats["iou"] * 100))
        print(" ".join(["{:.4f}, "] * args.classes).format(*(stats["iou_ssc"] * 100).tolist()))
        print("mIoU={:.4f}".format(stats["iou_ssc_mean"] * 100))
    if args.frames_out:
        if "pred" not in maps:
            raise SystemExit("--frames-out samples the prediction map: give --pred")
        sample_frames(maps["pred"], poses, args, device)
    return maps, stats


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--poses", required=True, help="the sequence directory with poses.txt and calib.txt")
    ap.add_argument("--pred", default=None)
    ap.add_argument("--gt", default=None)
    ap.add_argument("--out", required=True, help="path prefix of the PLY files")
    ap.add_argument("--min-obs", type=int, default=1)
    ap.add_argument("--every", type=int, default=1, help="use every n-th frame")
    ap.add_argument("--min-component", type=int, default=0, metavar="N",
                    help="prediction frames: connected components (26) of the things classes 1-8 of fewer than N voxels do not vote")
    ap.add_argument("--fov", action="store_true", help="pickles: vote inside the frame's fov_mask_1 only")
    ap.add_argument("--dims", type=int, nargs=3, default=(256, 256, 32))
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, -25.6, -2.0))
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--max-bricks", type=int, default=None)
    ap.add_argument("--views", nargs="*", default=[], choices=render.MAP_VIEW_NAMES,
                    help="draw the map: <out>_{pred,gt,err}_{view}.png (render.render_map)")
    ap.add_argument("--png-side", type=int, default=render.MAP_BEV_SIDE, help="longest side of the bev picture, pixels")
    ap.add_argument("--camera-every", type=int, default=0,
                    help="draw the map through the left colour camera (P2, Tr of calib.txt) of every n-th posed frame")
    ap.add_argument("--camera-size", type=int, nargs=2, default=(370, 1220), help="H W of the camera pictures")
    ap.add_argument("--t-max", type=float, default=80.0, help="camera pictures: voxels deeper than this (m) are not drawn")
    ap.add_argument("--mesh", action="store_true",
                    help="write the maps' surfaces as indexed quad meshes: <out>_{pred,gt}_mesh.ply (occdepth_amd.mesh)")
    ap.add_argument("--mesh-open", action="store_true",
                    help="--mesh: leave out the faces towards unobserved space (only where observed free space meets matter)")
    ap.add_argument("--frames-out", default=None,
                    help="read the prediction map back into every --pred frame: DIR/sequences/<seq>/predictions/<frame>.label")
    ap.add_argument("--exclude-self", action="store_true", help="--frames-out: take the frame's own vote out of the map first")
    ap.add_argument("--keep-own", action="store_true", help="--frames-out: a tie that the frame's own label is part of goes to it")
    ap.add_argument("--visibility", type=int, nargs=2, default=None, metavar=("W_VIS", "W_HID"),
                    help="occlusion-aware votes of the prediction map: a voxel the left camera's pixel rays reach in the frame's "
                         "own labels votes with W_VIS (1..255), any other with W_HID (0..255); camera from calib.txt and --camera-size")
    ap.add_argument("--frame-range", type=int, nargs=2, default=None, metavar=("FIRST", "LAST"), help="use these frames only (inclusive)")
    ap.add_argument("--save-map", default=None, metavar="PREFIX", help="keep the maps' vote counters: PREFIX_{pred,gt}.occmap")
    ap.add_argument("--load-map", nargs="+", default=None, metavar="PREFIX",
                    help="merge PREFIX_{pred,gt}.occmap of earlier runs in before the frames are integrated")
    return ap


if __name__ == "__main__":
    if not torch.cuda.is_available():
        raise SystemExit("map_sequence.py builds the map on the GPU; there is none here")
    run(parser().parse_args())
