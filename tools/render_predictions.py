"""Render the pickles scripts/generate_output.py (occdepth_amd.output.write_outputs) writes to PNG, on the GPU and without
a display: the headless replacement for the reference's scripts/visualization/kitti_vis_pred.py, kitti_vis_pred_batch.py
and NYU_vis_pred.py.

    python tools/render_predictions.py <dir of .pkl> [--out DIR] [--dataset kitti|NYU] [--views camera bev oblique]
                                       [--image-size H W] [--target] [--batch 8] [--mesh] [--min-component N] [--instances]

Every <name>.pkl gives <name>_<view>.png next to it, or under --out with the same sub-directories.  Pickle keys: `y_pred`
(X, Y, Z), `fov_mask_1` (dims voxels outside are dimmed), `cam_k`, `T_velo_2_cam` (kitti), `cam_pose`, `vox_origin` (NYU);
--target colours the prediction against the pickle's `target` (error mode).  Frames are batched per launch.  --mesh also writes <name>_mesh.ply, the frame's surface as an indexed quad
mesh in world metres (occdepth_amd/mesh.py, K39).  --min-component N removes the connected components (26-connectivity) of
the dataset's things classes that have fewer than N voxels before anything is drawn or meshed; --instances colours the things
voxels by component instead of by class (occdepth_amd/panoptic.py, K40).
"""
import argparse
import os
import pickle
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import render  # noqa: E402

IMAGE_SIZE = {"kitti": (370, 1220), "NYU": (480, 640)}
VOXEL_METRES = {"kitti": 0.2, "NYU": 0.08}
FULL_X = {"kitti": 256, "NYU": 60}


def find_pickles(root):
    out = []
    for d, _, files in sorted(os.walk(root)):
        out += [os.path.join(d, f) for f in sorted(files) if f.endswith(".pkl")]
    return out


def render_group(paths, frames, args, dev):
    """One launch for frames of one grid shape -> the written paths."""
    labels = torch.from_numpy(np.stack([np.asarray(f["y_pred"]).astype(np.int16) for f in frames])).to(dev)
    min_component, instances = int(getattr(args, "min_component", 0) or 0), bool(getattr(args, "instances", False))
    drawn = labels
    if min_component > 1 or instances:
        labels, drawn = component_labels(labels, args.dataset, min_component, instances)
    B = labels.shape[0]
    dims = tuple(int(d) for d in labels.shape[1:])
    vs = args.voxel_size or VOXEL_METRES[args.dataset] * FULL_X[args.dataset] / dims[0]

    def camera():
        batch = {k: [f[k] for f in frames] for k in ("cam_k", "T_velo_2_cam", "cam_pose", "vox_origin") if k in frames[0]}
        origin = (0.0, -0.5 * vs * dims[1], -2.0) if args.dataset == "kitti" else None
        k, E, origin = render.batch_camera(batch, args.dataset, origin, dev)
        return render.camera_view(k, E, origin, vs), tuple(args.image_size or IMAGE_SIZE[args.dataset])

    views, sizes = render.standard_views(args.views, dims, dev, camera)
    fov = None
    if all("fov_mask_1" in f for f in frames):
        n = dims[0] * dims[1] * dims[2]
        rows = [np.asarray(f["fov_mask_1"]) for f in frames]
        if all(r.size >= n and r.size % n == 0 for r in rows):
            # (N,), (N, 1), or the loader's (V, N, P): left view, pattern point 0
            fov = torch.from_numpy(np.stack([r.reshape(-1)[:n] if r.size == n else r.reshape(r.shape[0], n, -1)[0, :, 0]
                                             for r in rows]).astype(bool)).to(dev).reshape(labels.shape)
    target = None
    if args.target:
        missing = [p for p, f in zip(paths, frames) if "target" not in f]
        if missing:
            raise SystemExit("--target: no `target` in %s" % missing[0])
        target = torch.from_numpy(np.stack([np.asarray(f["target"]).astype(np.int16) for f in frames])).to(dev)
    images = render.render_labels(labels if args.target else drawn, views, sizes, fov=fov, target=target, mode="error" if args.target else "class",
                                  palette=args.dataset)
    host = [t.cpu().numpy() for t in images]
    written = []
    for i, p in enumerate(paths):
        stem = os.path.splitext(p)[0]
        if args.out:
            stem = os.path.join(args.out, os.path.relpath(stem, args.root))
            os.makedirs(os.path.dirname(stem), exist_ok=True)
        for name, h in zip(args.views, host):
            written.append(render.write_png("%s_%s.png" % (stem, name), h[i]))
        if args.mesh:
            written.append(write_frame_mesh(stem, labels[i], frames[i], vs, args.dataset))
    return written


def component_labels(labels, dataset, min_component=0, instances=False, connectivity=26):
    """--min-component / --instances: labels (B, X, Y, Z) int16 -> (the labels with every component of a things class of
    fewer than min_component voxels set to 0, the labels to draw).  With instances the drawn label of a things voxel is a
    palette row chosen by a fixed integer hash of its segment's compact id, 1 + (id * 2654435761 mod 2^32 >> 16) mod
    (n_classes - 1), instead of its class (occdepth_amd.panoptic, K40)."""
    from occdepth_amd import hip, panoptic
    things, _ = panoptic.default_classes(dataset)
    lab8 = torch.where((labels < 0) | (labels > 255), torch.full_like(labels, 255), labels).to(torch.uint8).contiguous()
    if min_component > 1:
        lab8 = hip.ccl_filter(lab8, things, min_component, connectivity)
    out = lab8.to(torch.int16)
    if not instances:
        return out, out
    ids, _, _, _ = hip.ccl_compact(hip.ccl_segments(lab8, things, (), connectivity), lab8)
    n = int(render.palette(dataset).shape[0]) - 3
    colour = 1 + (((ids.long() * 2654435761) & 0xFFFFFFFF) >> 16) % (n - 1)
    return out, torch.where(ids > 0, colour.to(torch.int16), out)


def write_frame_mesh(stem, labels, frame, vs, dataset):
    """--mesh: <stem>_mesh.ply, the closed surface of one frame's prediction (occdepth_amd.mesh.mesh_labels, K39) -> the path."""
    from occdepth_amd import mesh
    if dataset == "kitti":
        origin = (0.0, -0.5 * vs * int(labels.shape[1]), -2.0)
    else:
        origin = np.asarray(frame["vox_origin"], dtype=np.float64).reshape(-1)[:3]
    part = mesh.mesh_labels(labels, vs, origin)
    return mesh.write_mesh_ply("%s_mesh.ply" % stem, part, render.palette(dataset))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("root")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dataset", default="kitti", choices=sorted(IMAGE_SIZE))
    ap.add_argument("--views", nargs="+", default=["camera", "bev"], choices=render.VIEW_NAMES)
    ap.add_argument("--image-size", nargs=2, type=int, default=None, metavar=("H", "W"),
                    help="size of the camera image the pickles' cam_k belongs to")
    ap.add_argument("--voxel-size", type=float, default=None, help="metres; default: the dataset's, from the grid's size")
    ap.add_argument("--target", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--mesh", action="store_true", help="also write every frame's surface as <name>_mesh.ply (occdepth_amd.mesh)")
    ap.add_argument("--min-component", type=int, default=0, metavar="N",
                    help="before drawing and meshing, remove every connected component of a things class of fewer than N voxels")
    ap.add_argument("--instances", action="store_true", help="colour things voxels by connected component instead of by class")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("render_predictions.py renders on the GPU; none is visible")
    dev = torch.device("cuda")
    paths = find_pickles(args.root)
    if not paths:
        raise SystemExit("no .pkl under %s" % args.root)
    written, group, frames = [], [], []

    def flush():
        if group:
            written.extend(render_group(list(group), list(frames), args, dev))
            group.clear()
            frames.clear()

    for p in paths:
        with open(p, "rb") as f:
            frame = pickle.load(f)
        if frames and (np.asarray(frame["y_pred"]).shape != np.asarray(frames[0]["y_pred"]).shape or len(group) >= args.batch):
            flush()
        group.append(p)
        frames.append(frame)
    flush()
    print("%d images from %d frames" % (len(written), len(paths)))
    return written


if __name__ == "__main__":
    main()
