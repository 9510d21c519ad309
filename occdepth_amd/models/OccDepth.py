"""OccDepth top module (mirror of occdepth/models/OccDepth.py:30-376, the forward hot path).

Constructor signature, config attributes read, sub-module names (`net_rgb`, `projects`,
`flosp_depth`, `net_3d_decoder`) and the `forward(batch) -> dict` contract are the reference's.
Forward without autograd (eval under torch.no_grad()):
    2-D UNet per view (PyTorch-ROCm / MIOpen + HIP helpers; both views in one batch, optionally replayed as a hipGraph)
 -> K1a FLoSP-Depth frustum sample + K1b fused multi-scale Stereo-SFA lift   (HIP, HBM-bound)
 -> channels-last 3-D UNet + CRP + cascade head on fp32-MFMA implicit GEMM     (HIP, MFMA-bound)
With autograd (training, or eval with gradients enabled) the reference's per-sample / per-scale structure runs on ATen
autograd, with the 3-D convolutions on the HIP forward / dgrad / wgrad kernels (autograd3d.py).  `step` and the
Lightning `*_step` hooks assemble the reference's losses from one statistics pass (loss/ssc_loss.py) and keep the
SSC metrics on the GPU.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..fused import needs_autograd
from ..train_graph import new_graph, seal_graph
from .SFA import SFA, lift_scales, lift_scales_proj
from .flosp_depth import flosp_depth_conf_map
from .flosp_depth.flosp_depth import FlospDepth
from .unet2d import UNet2D
from .unet3d_kitti import UNet3D as UNet3DKitti
from .unet3d_nyu import UNet3D as UNet3DNYU

# hipStreamCaptureModeThreadLocal: only the capturing thread's calls are checked, so a process group's watchdog thread
# (event queries) cannot invalidate -- or abort -- a capture running beside it (N > 1 ranks, OCCDEPTH_FORCE_DIST=1)
CAPTURE_MODE = "thread_local"

try:  # the reference's base class; absent in this image -> plain nn.Module with the hooks it uses
    import pytorch_lightning as pl
    _Base = pl.LightningModule
except Exception:  # pragma: no cover - depends on the environment
    class _Base(nn.Module):
        def save_hyperparameters(self, *a, **k):
            pass

        def log(self, *a, **k):
            pass

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class OccDepth(_Base):
    def __init__(self, class_names, class_weights, class_weights_occ=None, full_scene_size=None, project_res=[],
                 config=None, infer_mode=False):
        super().__init__()
        self.project_res = project_res
        self.full_scene_size = full_scene_size
        self.class_names = class_names
        self.class_weights = class_weights
        self.class_weights_occ = class_weights_occ
        for key in ("dataset", "frustum_size", "project_scale", "n_relations", "lr", "weight_decay", "fp_loss",
                    "context_prior", "relation_loss", "CE_ssc_loss", "sem_scal_loss", "geo_scal_loss", "n_classes",
                    "feature", "feature_2d_oc", "trans_2d_to_3d", "cascade_cls", "occluded_cls",
                    "sem_step_decay_loss", "multi_view_mode", "share_2d_backbone_gradient", "use_stereo_depth_gt",
                    "use_lidar_depth_gt", "use_depth_gt"):
            setattr(self, key, getattr(config, key))
        print("INFO: Use cascade cls: {}".format(self.cascade_cls))
        print("INFO: Use occluded cls: {}".format(self.occluded_cls))
        self.infer_mode = infer_mode
        # eval fast path, OFF by default (the default forward is the reference's: per-view 2-D passes, fresh tensors).
        # `enable_fast_eval()` -- or OCCDEPTH_FAST_EVAL=1 in the environment of an unmodified scripts/eval.py /
        # generate_output.py run -- switches all three on; the individual variables switch them one by one.
        env = os.environ.get
        fast = env("OCCDEPTH_FAST_EVAL", "0") == "1"
        self.batch_views = fast or env("OCCDEPTH_BATCH_VIEWS", "0") == "1"   # all views through net_rgb as one batch
        self.graph_2d = self.batch_views and (fast or env("OCCDEPTH_GRAPH_2D", "0") == "1")    # 2-D network as one hipGraph
        self.graph_all = self.batch_views and (fast or env("OCCDEPTH_GRAPH_ALL", "0") == "1")  # WHOLE forward as one hipGraph
        # graph_all replays into static output buffers; by default the caller gets fresh tensors (the reference's contract:
        # a caller may keep `pred` across forwards).  False hands out the static buffers themselves (valid until the next
        # forward of this model) and saves the ~0.1 ms copy of ~300 MB at config 2.
        self.clone_graph_outputs = env("OCCDEPTH_CLONE_OUTPUTS", "1") == "1"
        self._graphs = {}
        self.batch_views_train = os.environ.get("OCCDEPTH_TRAIN_BATCH_VIEWS", "1") == "1"
        # training fast path, OFF by default (the default `training_step` returns the loss and the Trainer runs backward and
        # the optimizer, as in the reference).  `enable_fast_train()` -- or OCCDEPTH_FAST_TRAIN=1 in the environment of an
        # unmodified scripts/train.py run -- switches the module to manual optimisation: `training_step` then replays the
        # WHOLE step (forward, losses, backward, gradient exchange, [gradient-norm clip +] AdamW) from one hipGraph (train_graph.GraphedTrainStep,
        # the step bench.py --train times).  OCCDEPTH_FAST_TRAIN_BF16=1: the bf16-MFMA convolution mode of configs[3].
        # OCCDEPTH_FAST_TRAIN_ACCUM=N: gradient accumulation over N micro-batches (`_accumulate_value`).
        self._fast_train = None
        self._opt = self._sched = None
        self.fast_train = False
        self.fast_train_grad_clip = None
        self.fast_train_accumulate = None
        if env("OCCDEPTH_FAST_TRAIN", "0") == "1":
            self.enable_fast_train(bf16=env("OCCDEPTH_FAST_TRAIN_BF16", "0") == "1")
        self.fused_lift = True    # training on the GPU: HIP lift + one-launch backward (lift_autograd.py) where it applies
        # Training targets built on the GPU (targets.py) instead of in the dataloader workers.  OCCDEPTH_GPU_TARGETS =
        #   auto (default)  build the frustum masks / class counts and the relation matrices a batch does NOT bring (key
        #                   absent, an empty list, or zero-element entries: what the hooked collate delivers); a batch
        #                   that brings them is used as it is;
        #   1               always build (the batch's targets are ignored) and rebind the reference dataset's two target
        #                   functions to stubs (targets.defer_dataset_targets; reaches dataloader workers forked later);
        #   0               never build.
        self.gpu_targets = {"1": True, "0": False}.get(env("OCCDEPTH_GPU_TARGETS", "auto"), "auto")
        self._dataset_hook = None
        if self.gpu_targets is True:
            from ..targets import defer_dataset_targets
            self._dataset_hook = defer_dataset_targets()
        # OCCDEPTH_GPU_PROJECTION=1: also take the voxel -> pixel tables out of the loader (targets.defer_dataset_projection
        # stubs its vox2pix); a batch without tables is projected on the GPU (occd_vox2pix), in training as in eval.  The
        # stub also silences compute_local_frustums, so the frustum targets must then come from the GPU builders.
        self._projection_hook = None
        if env("OCCDEPTH_GPU_PROJECTION", "0") == "1":
            if self.gpu_targets is False:
                raise ValueError("OCCDEPTH_GPU_PROJECTION=1 stubs the loader's compute_local_frustums: it needs the GPU "
                                 "training targets (OCCDEPTH_GPU_TARGETS=auto or 1), not OCCDEPTH_GPU_TARGETS=0")
            from ..targets import defer_dataset_projection
            self._projection_hook = defer_dataset_projection()
        # OCCDEPTH_GPU_STEREO=1: the stereo depth target (`gt_depth` of use_stereo_depth_gt) is matched on the GPU from the
        # batch's own image pair (`enable_stereo_depth`, stereo.py) whenever the batch brings none, and the loader's
        # `load_depth` is rebound to a stub (targets.defer_dataset_stereo_depth), so no depth PNG is read.  OFF by default:
        # nothing is allocated or launched.  OCCDEPTH_GPU_STEREO_DISP: the number of disparities (192).
        self.gpu_stereo = None
        self._stereo_hook = None
        if env("OCCDEPTH_GPU_STEREO", "0") == "1":
            self.enable_stereo_depth(max_disp=int(env("OCCDEPTH_GPU_STEREO_DISP", "192")))
            from ..targets import defer_dataset_stereo_depth
            self._stereo_hook = defer_dataset_stereo_depth()
        if infer_mode:
            self.context_prior = False
        assert not (config.use_stereo_depth_gt and config.use_lidar_depth_gt), "only with one depth data supported."
        self.with_depth_gt = self.use_stereo_depth_gt or self.use_lidar_depth_gt or self.use_depth_gt
        self.depth_loss_w = config.depth_loss_weight

        if self.dataset == "NYU":
            self.net_3d_decoder = UNet3DNYU(self.n_classes, nn.BatchNorm3d, n_relations=self.n_relations,
                                            feature=self.feature, full_scene_size=self.full_scene_size,
                                            context_prior=self.context_prior, cascade_cls=self.cascade_cls,
                                            infer_mode=self.infer_mode)
        elif self.dataset == "kitti":
            self.net_3d_decoder = UNet3DKitti(self.n_classes, nn.BatchNorm3d, project_scale=self.project_scale,
                                              feature=self.feature, full_scene_size=self.full_scene_size,
                                              context_prior=self.context_prior, cascade_cls=self.cascade_cls,
                                              occluded_cls=self.occluded_cls, infer_mode=self.infer_mode)
        self.net_rgb = UNet2D.build(out_feature=self.feature_2d_oc, use_decoder=True,
                                    backbone_2d_name=config.backbone_2d_name,
                                    return_up_feats=config.return_up_feats)
        self.save_hyperparameters()
        from ..loss.sscMetrics import SSCMetrics
        self.train_metrics = SSCMetrics(self.n_classes)      # reference :131-133 (confusion matrices live on the GPU here)
        self.val_metrics = SSCMetrics(self.n_classes)
        self.test_metrics = SSCMetrics(self.n_classes)
        self.metrics_allreduce = False    # opt-in: sum the confusion matrices over ranks before the epoch statistics
        # Evaluation report by region (camera FOV, range boxes, per frame), OFF by default: `enable_eval_report()` -- or
        # OCCDEPTH_EVAL_REPORT=kitti in the environment of an unmodified scripts/eval.py.  Off: nothing is allocated or launched.
        self.eval_report = None
        self.report_metrics = {}
        if env("OCCDEPTH_EVAL_REPORT", ""):
            self.enable_eval_report(env("OCCDEPTH_EVAL_REPORT"))
        # Qualitative frames (render.py: predictions ray-cast to PNG on the GPU), OFF by default: `enable_render()` -- or
        # OCCDEPTH_RENDER_DIR=<dir> [OCCDEPTH_RENDER_EVERY=n] [OCCDEPTH_RENDER_MODE=class|error] in the environment of an
        # unmodified scripts/eval.py.  Off: nothing is allocated or launched.
        self.render = None
        if env("OCCDEPTH_RENDER_DIR", ""):
            self.enable_render(env("OCCDEPTH_RENDER_DIR"), every=int(env("OCCDEPTH_RENDER_EVERY", "1")),
                               mode=env("OCCDEPTH_RENDER_MODE", "class"))
        # Temporal fusion of the test / validation predictions over a sequence (fuse.py), OFF by default:
        # `enable_temporal_fusion()` -- or OCCDEPTH_FUSE=<window> OCCDEPTH_FUSE_POSES=<.../dataset/sequences>
        # [OCCDEPTH_FUSE_DECAY=d] in the environment of an unmodified scripts/eval.py.  Off: nothing is imported, allocated
        # or launched.
        self.temporal_fusion = None
        self.fused_metrics = {}
        if env("OCCDEPTH_FUSE", "0") not in ("", "0"):
            self.enable_temporal_fusion(env("OCCDEPTH_FUSE_POSES", ""), window=int(env("OCCDEPTH_FUSE")),
                                        decay=float(env("OCCDEPTH_FUSE_DECAY", "1.0")))
        # Sequence-level semantic map of the test / validation frames (semantic_map.py), OFF by default:
        # `enable_semantic_map()` -- or OCCDEPTH_MAP_DIR=<dir> OCCDEPTH_MAP_POSES=<.../dataset/sequences> (falls back to
        # OCCDEPTH_FUSE_POSES) [OCCDEPTH_MAP_MIN_OBS=n] [OCCDEPTH_MAP_VIEWS=bev,oblique] [OCCDEPTH_MAP_FRAMES=1 [OCCDEPTH_MAP_FRAMES_SELF=0]
        # [OCCDEPTH_MAP_SUBMISSION=<dir>]: the map read back into every frame] [OCCDEPTH_MAP_GATHER=0] [OCCDEPTH_MAP_SAVE=1] in the environment of an unmodified scripts/eval.py.  Off: nothing is
        # imported, allocated or launched.  Every other method reaches it through getattr(self, "semantic_map", None).
        # [OCCDEPTH_MAP_VISIBILITY=<w_vis>,<w_hid>]: the prediction map takes occlusion-aware votes (visibility.py, K34).
        # [OCCDEPTH_MAP_MESH=1]: every sequence's maps also leave as surface meshes (mesh.py, K39).
        self.semantic_map = None
        if env("OCCDEPTH_MAP_DIR", ""):
            weights = env("OCCDEPTH_MAP_VISIBILITY", "")
            self.enable_semantic_map(env("OCCDEPTH_MAP_DIR"), env("OCCDEPTH_MAP_POSES", "") or env("OCCDEPTH_FUSE_POSES", ""),
                                     min_obs=int(env("OCCDEPTH_MAP_MIN_OBS", "1")),
                                     views=tuple(v for v in env("OCCDEPTH_MAP_VIEWS", "").split(",") if v),
                                     frames=env("OCCDEPTH_MAP_FRAMES", "0") == "1",
                                     submission_dir=env("OCCDEPTH_MAP_SUBMISSION", "") or None,
                                     exclude_self=env("OCCDEPTH_MAP_FRAMES_SELF", "1") == "0",
                                     gather=env("OCCDEPTH_MAP_GATHER", "1") != "0", save_maps=env("OCCDEPTH_MAP_SAVE", "0") == "1",
                                     visibility=tuple(int(w) for w in weights.split(",")) if weights else None,
                                     mesh=env("OCCDEPTH_MAP_MESH", "0") == "1")
        # RayIoU of the test / validation predictions (ray_metric.py, K35), OFF by default: `enable_ray_metrics()` -- or
        # OCCDEPTH_RAY_METRIC=1 [OCCDEPTH_RAY_ORIGINS=<n>[,<step>]] [OCCDEPTH_RAY_POSES=<.../dataset/sequences>] (falls back
        # to OCCDEPTH_FUSE_POSES) [OCCDEPTH_RAY_UNKNOWN=pass] in the environment of an unmodified scripts/eval.py.  Off:
        # nothing is imported, allocated or launched.  Every other method reaches it through getattr(self, "ray_metrics", None).
        self.ray_metrics = None
        if env("OCCDEPTH_RAY_METRIC", "0") == "1":
            spec = env("OCCDEPTH_RAY_ORIGINS", "1").split(",")
            if len(spec) not in (1, 2) or not all(w.strip().isdigit() for w in spec):
                raise ValueError("OCCDEPTH_RAY_ORIGINS is <n>[,<step>], got %r" % env("OCCDEPTH_RAY_ORIGINS"))
            self.enable_ray_metrics(origins=int(spec[0]), origin_step=int(spec[1]) if len(spec) == 2 else 5,
                                    poses_root=env("OCCDEPTH_RAY_POSES", "") or env("OCCDEPTH_FUSE_POSES", "") or None,
                                    unknown=env("OCCDEPTH_RAY_UNKNOWN", "drop") or "drop")
        # Distance-tolerant scores of the test / validation predictions (dist_metric.py, K37), OFF by default:
        # `enable_distance_metrics()` -- or OCCDEPTH_DIST_METRIC=1 [OCCDEPTH_DIST_THRESHOLDS=<m>[,<m>...]] [OCCDEPTH_DIST_FOV=1]
        # in the environment of an unmodified scripts/eval.py.  Off: nothing is imported, allocated or launched.  Every
        # other method reaches it through getattr(self, "dist_metrics", None).
        self.dist_metrics = None
        if env("OCCDEPTH_DIST_METRIC", "0") == "1":
            spec = env("OCCDEPTH_DIST_THRESHOLDS", "") or "0.2,0.4,0.8"
            try:
                thresholds = tuple(float(w) for w in spec.split(","))
            except ValueError:
                raise ValueError("OCCDEPTH_DIST_THRESHOLDS is <metres>[,<metres>...], got %r" % spec) from None
            self.enable_distance_metrics(thresholds_m=thresholds, fov_only=env("OCCDEPTH_DIST_FOV", "0") == "1")
        # Panoptic quality of the test / validation predictions (panoptic.py, K40), OFF by default:
        # `enable_panoptic_metrics()` -- or OCCDEPTH_PANOPTIC=1 [OCCDEPTH_PANOPTIC_MIN_VOXELS=<n>]
        # [OCCDEPTH_PANOPTIC_CONNECTIVITY=6|26] [OCCDEPTH_PANOPTIC_FOV=1] in the environment of an unmodified scripts/eval.py.
        # Off: nothing is imported, allocated or launched.  Every other method reaches it through
        # getattr(self, "panoptic_metrics", None).
        self.panoptic_metrics = None
        if env("OCCDEPTH_PANOPTIC", "0") == "1":
            spec = (env("OCCDEPTH_PANOPTIC_MIN_VOXELS", "") or "1", env("OCCDEPTH_PANOPTIC_CONNECTIVITY", "") or "26")
            if not all(w.strip().isdigit() for w in spec):
                raise ValueError("OCCDEPTH_PANOPTIC_MIN_VOXELS and OCCDEPTH_PANOPTIC_CONNECTIVITY are integers, got %r, %r" % spec)
            self.enable_panoptic_metrics(connectivity=int(spec[1]), min_pred_voxels=int(spec[0]),
                                         fov_only=env("OCCDEPTH_PANOPTIC_FOV", "0") == "1")
        self.init_2d_to_3d_trans(config)
        # `enable_render_loss()` -- or OCCDEPTH_RENDER_LOSS=<weight>[,<stride>] in the environment of an unmodified
        # scripts/train.py: the depth-rendering loss (loss/render_loss.py, K36) -- `ssc_logit` composited along the left
        # camera's pixel rays into an expected depth image, held to the step's `gt_depth` (the batch's, or the one
        # `enable_stereo_depth` matches) -- is added to the train / val loss.  Off: nothing is imported, allocated or launched.
        self.render_loss = None
        if env("OCCDEPTH_RENDER_LOSS", "0") not in ("", "0"):
            spec = env("OCCDEPTH_RENDER_LOSS").split(",")
            try:
                if len(spec) > 2:
                    raise ValueError
                weight, stride = float(spec[0]), int(spec[1]) if len(spec) > 1 else 4
            except ValueError:
                raise ValueError("OCCDEPTH_RENDER_LOSS is <weight>[,<stride>], got %r" % env("OCCDEPTH_RENDER_LOSS")) from None
            self.enable_render_loss(weight=weight, stride=stride)
        # `enable_lovasz_loss()` -- or OCCDEPTH_LOVASZ=<weight> in the environment of an unmodified scripts/train.py: the
        # Lovasz-softmax loss (loss/lovasz_loss.py, on the K38 sort), the surrogate of the per-class Jaccard index, is added
        # to the train / val loss.  Off: nothing is imported, allocated or launched.
        self.lovasz_loss = None
        if env("OCCDEPTH_LOVASZ", "0") not in ("", "0"):
            try:
                weight = float(env("OCCDEPTH_LOVASZ"))
            except ValueError:
                raise ValueError("OCCDEPTH_LOVASZ is <weight>, got %r" % env("OCCDEPTH_LOVASZ")) from None
            self.enable_lovasz_loss(weight=weight)
        print("INFO: Use step decay loss: {}".format(self.sem_step_decay_loss))
        batch_size = config.batch_size_per_gpu * config.n_gpus
        if self.dataset == "kitti":
            self.total_batch = (3834 // batch_size) * 30
        elif self.dataset == "NYU":
            self.total_batch = (795 // batch_size) * 30
        else:
            raise NotImplementedError(self.dataset)
        self.cur_batch = 0

    def init_2d_to_3d_trans(self, config):
        print("INFO: Selected 2d->3d transformation method: {}".format(self.trans_2d_to_3d))
        if self.trans_2d_to_3d not in ("flosp", "flosp_depth"):
            raise NotImplementedError(f"{self.trans_2d_to_3d} is not supported yet.")
        self.scale_2ds = [1, 2, 4, 8]
        self.projects = nn.ModuleDict({
            str(s): SFA(config.full_scene_size, project_scale=self.project_scale, dataset=self.dataset)
            for s in self.scale_2ds})
        if self.trans_2d_to_3d == "flosp_depth":
            conf = dict(flosp_depth_conf_map[self.dataset])
            conf.update({
                "scene_size": config.full_scene_size,
                "project_scale": config.project_scale,
                "output_channels": config.feature,
                "depth_net_conf": dict(in_channels=config.feature,
                                       mid_channels=conf["depth_net_conf"]["mid_channels"]),
                "return_depth": self.with_depth_gt,
                "infer_mode": self.infer_mode,
            })
            self.flosp_depth_conf = conf
            self.flosp_depth = FlospDepth(**conf)
            if self.with_depth_gt:
                from ..loss.depth_loss import DepthClsLoss
                self.depth_loss_fn = DepthClsLoss(downsample_factor=conf["downsample_factor"], d_bound=conf["d_bound"])

    # ---------------------------------------------------------------- 2-D side
    def _stamp_of(self, root, slot):
        """Exact fingerprint of every tensor a captured graph bakes pointers / folded copies of: in-place updates
        (optimizer.step, load_state_dict) bump `_version`; replaced storage changes `data_ptr`.  Tuples, not sums (a sum
        can collide); the tensor list is cached until train() / _apply() / load_state_dict() drop the graphs."""
        ts = self.__dict__.get(slot)
        if ts is None:
            ts = list(root.parameters()) + list(root.buffers())
            self.__dict__[slot] = ts
        return (tuple([t._version for t in ts]), tuple([t.data_ptr() for t in ts]))

    def _net_rgb_stamp(self):
        return self._stamp_of(self.net_rgb, "_net_rgb_tensors")

    def _drop_graphs(self):
        self._graphs.clear()
        self.__dict__.pop("_net_rgb_tensors", None)
        self.__dict__.pop("_all_tensors", None)

    def enable_fast_eval(self, clone_outputs=True, graph=True):
        """Switch the eval forward to the benched configuration: both views through the 2-D network as one batch and the
        whole forward replayed from ONE captured hipGraph (`graph=False`: batched views only).  `clone_outputs=True` (default)
        returns fresh tensors per call like the reference; False returns the graph's static output buffers, valid until the
        next forward.  The same switches from the environment: OCCDEPTH_FAST_EVAL=1 (OCCDEPTH_CLONE_OUTPUTS=0)."""
        self.batch_views = True
        self.graph_2d = self.graph_all = bool(graph)
        self.clone_graph_outputs = bool(clone_outputs)
        self._drop_graphs()
        return self

    def enable_fast_train(self, bf16=False, autocast=False, grad_clip=None, accumulate=None):
        """Manual optimisation + the whole training step as ONE replayed hipGraph (see `_fast_training_step`).  Call before
        `trainer.fit` (Lightning reads `automatic_optimization` when the loop starts).  `grad_clip`: global gradient-norm
        clip for callers without a Trainer (0 = none); left at None, the attached Trainer's `gradient_clip_val` is used
        (`_grad_clip_value`) -- under manual optimisation Lightning itself no longer clips.  `accumulate`: gradient
        accumulation over N micro-batches; left at None, OCCDEPTH_FAST_TRAIN_ACCUM, then the Trainer's
        `accumulate_grad_batches` (`_accumulate_value`) -- which Lightning skips too under manual optimisation."""
        if accumulate is not None:
            self._check_accumulate(accumulate, "enable_fast_train(accumulate=...)")
        self.fast_train = True
        self.fast_train_grad_clip = grad_clip
        self.fast_train_accumulate = accumulate
        self.fast_train_bf16, self.fast_train_autocast = bool(bf16), bool(autocast)
        self.automatic_optimization = False
        self._fast_train = None
        return self

    def invalidate_graphs(self):
        """Forget every captured hipGraph (they are re-captured on the next forward / training step)."""
        self._drop_graphs()
        self._fast_train = None

    def train(self, mode=True):
        self._drop_graphs()
        return super().train(mode)

    def _apply(self, fn, *a, **k):
        self._drop_graphs()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._drop_graphs()
        return super().load_state_dict(*a, **k)

    # Round 6 experiment (OCCDEPTH_DEPTHNET_OVERLAP=1): FLoSP-Depth's DepthNet (seven 3x3 convolutions + gate + softmax on the 1/8
    # map: ~0.45 ms of 120-workgroup launches) only needs the 1/8 feature, which the decoder has after its second level; started
    # on a side stream there, it runs beside the 1/4, 1/2 and 1/1 levels (~5 ms of chip-filling launches) instead of after them.
    # Captured into the whole-forward hipGraph as a parallel branch (fork = the decoder's callback, join = in front of the lift).
    depthnet_overlap = os.environ.get("OCCDEPTH_DEPTHNET_OVERLAP", "0") == "1"

    def _depthnet_hook(self, batch, img, bs, n_views):
        """The decoder callback that launches `_depth_volume` early, or None when the conditions of the fused eval lift (the only
        consumer of a deferred frustum) do not hold."""
        if not (self.depthnet_overlap and self.trans_2d_to_3d == "flosp_depth" and self.dataset == "kitti" and img.is_cuda
                and not needs_autograd(self)):
            return None
        if self._lift_calibration(batch, img, "projected_pix_{}".format(self.project_scale)) is None:
            return None
        layer = "1_{}".format(self.flosp_depth_conf["downsample_factor"])
        want = int(self.flosp_depth_conf["downsample_factor"])

        def hook(s, feat):
            if s != want:
                return
            cur = torch.cuda.current_stream(feat.device)
            side = self.__dict__.get("_depth_stream")
            if side is None or side.device != feat.device:
                side = self.__dict__["_depth_stream"] = torch.cuda.Stream(device=feat.device)
            side.wait_stream(cur)                              # fork: everything up to the 1/8 feature head
            feat.record_stream(side)
            with torch.cuda.stream(side):
                views = feat.reshape(bs, n_views, *feat.shape[1:])
                x_rgb = [{layer: views[:, i]} for i in range(n_views)]
                self.__dict__["_early_depth"] = self._depth_volume(batch, x_rgb, None, defer_sample=True)
        return hook

    def _net_rgb_graphed(self, x, on_scale=None):
        """The 2-D network is ~1200 launches of mostly 5-40 us kernels: with `graph_2d` (opt-in, eval only) it is
        captured once per input shape into a hipGraph and replayed, so the host never gates the GPU there.  The 3-D
        stack stays outside (its launches are few, long, and individually timed by bench.py).  A captured graph holds
        pointers to the weights AND to tensors derived from them (folded BatchNorm, packed / Winograd-domain weights);
        every entry therefore carries a stamp of the network's tensors and is re-captured when it no longer matches
        (train(), load_state_dict() and device / dtype moves drop the cache outright)."""
        if not self.graph_2d or not x.is_cuda or torch.cuda.is_current_stream_capturing():
            # (inside the whole-forward capture the network is part of it)
            return self.net_rgb(x) if on_scale is None else self.net_rgb(x, on_scale=on_scale)
        key = (tuple(x.shape), x.device)
        stamp = self._net_rgb_stamp()
        entry = self._graphs.get(key)
        if entry is not None and entry[3] != stamp:
            entry = None
        if entry is None:
            static_in = x.clone()
            try:
                side = torch.cuda.Stream(device=x.device)
                side.wait_stream(torch.cuda.current_stream(x.device))
                with torch.cuda.stream(side):
                    for _ in range(2):                         # warm-up: lazy initialisation, weight caches, MIOpen solvers
                        self.net_rgb(static_in)
                torch.cuda.current_stream(x.device).wait_stream(side)
                graph = new_graph()
                with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
                    static_out = self.net_rgb(static_in)
                seal_graph(graph)
                entry = (graph, static_in, static_out, stamp)
            except (RuntimeError, torch.AcceleratorError) as e:   # capture is an optimisation, never a requirement
                import warnings
                warnings.warn(f"occdepth_amd: hipGraph capture of the 2-D network failed ({e!r}); running eagerly")
                self.graph_2d = False
                self.graph_2d_error = repr(e)
                torch.cuda.synchronize(x.device)
                return self.net_rgb(x)
            self._graphs[key] = entry
        graph, static_in, static_out, _ = entry
        static_in.copy_(x)
        graph.replay()
        return static_out

    def process_rgbs(self, img, batch, n_views):
        bs = img.shape[0]
        if not needs_autograd(self) and self.batch_views and n_views > 1:
            # eval: BN uses running stats, so the views can share one batched pass (opt-in: a different
            # conv batch size changes backend algorithm choice and hence fp32 round-off)
            self.__dict__.pop("_early_depth", None)
            both = self._net_rgb_graphed(img.reshape(bs * n_views, *img.shape[2:]),
                                         on_scale=self._depthnet_hook(batch, img, bs, n_views))
            x_rgb = [{k: v.reshape(bs, n_views, *v.shape[1:])[:, i] for k, v in both.items()}
                     for i in range(n_views)]
        elif self.training and self.batch_views_train and n_views > 1 and not self.share_2d_backbone_gradient:
            # training: both views through the 2-D network as ONE view-major batch with per-view BatchNorm statistics
            # (bn.view_groups) -- the numbers of the reference's per-view loop, half the launches and no gradient
            # accumulation kernels for the shared parameters
            from .. import bn as bn_mod
            stacked = img.transpose(0, 1).reshape(n_views * bs, *img.shape[2:])
            with bn_mod.view_groups(n_views):
                both = self.net_rgb(stacked)
            x_rgb = [{k: v[i * bs:(i + 1) * bs] for k, v in both.items()} for i in range(n_views)]
        else:
            x_rgb = [self.net_rgb(img[:, 0])]
            for i in range(1, n_views):
                if self.share_2d_backbone_gradient:
                    with torch.no_grad():
                        x_rgb.append(self.net_rgb(img[:, i]))
                else:
                    x_rgb.append(self.net_rgb(img[:, i]))
        if n_views == 1 and "gt_depth" in batch:
            bf = batch["virtual_bf"][0].to(device) if "virtual_bf" in batch else None
            x_rgb.append({"1_" + str(s): self.generate_virtual_img(batch, x_rgb[0]["1_" + str(s)], s, bf)
                          for s in self.project_res})
            n_views = 2
        return x_rgb, n_views

    def generate_virtual_img(self, batch, x_single_rgb, scale_2d, bf):
        """Virtual right view: shift the sampling grid by the disparity bf / depth (reference :233-260,
        including its use of sample 0's disparity for the whole batch)."""
        depth = batch["gt_depth"].to(device)
        n, c, h, w = x_single_rgb.shape
        depth_s = F.interpolate(depth, size=(h, w), mode="bilinear", align_corners=False)
        dx = torch.div(bf / int(scale_2d), depth_s).type_as(x_single_rgb)
        dx = torch.where(torch.isinf(dx), torch.zeros_like(dx), dx)
        ys = torch.arange(-1, 1, 2 / h)
        xs = torch.arange(-1, 1, 2 / w)
        gy, gx = torch.meshgrid(ys, xs, indexing="ij")
        grid = torch.stack((gx, gy), dim=2).unsqueeze(0).repeat(n, 1, 1, 1).to(device).type_as(dx)
        grid[..., 0] = grid[..., 0] + (dx * 2 / w)[0]
        return F.grid_sample(x_single_rgb, grid, mode="bilinear", padding_mode="border", align_corners=False)

    # ---------------------------------------------------------------- 2D -> 3D
    def _depth_volume(self, batch, x_rgb, vox_origin, defer_sample=False):
        layer = "1_{}".format(self.flosp_depth_conf["downsample_factor"])
        n_views = 1 if self.dataset == "NYU" else len(x_rgb)
        img_feat = torch.stack([x_rgb[j][layer] for j in range(n_views)], 1).to(device)
        if self.infer_mode:
            kw = {"img_feat": img_feat, "grids": batch["grids"], "scaled_pixel_size": batch["scaled_pixel_size"]}
        else:
            kw = {"img_feat": img_feat, "cam_k": batch["cam_k"], "T_velo_2_cam": batch["T_velo_2_cam"],
                  "ida_mats": batch["ida_mats"], "vox_origin": vox_origin}
        if defer_sample:
            kw["defer_sample"] = True
        if self.with_depth_gt:
            return self.flosp_depth(**kw)
        return self.flosp_depth(**kw), None

    # The eval lift can project the voxels and sample the depth frustum inside the kernel (csrc/lift.hip lift_proj_kernel)
    # from the batch's calibration -- no voxel->pixel tables read.  `lift_in_kernel`:
    #   "auto"  (default) when the batch carries NO `projected_pix_{s}` / `fov_mask_{s}` tables (nothing to contradict: the
    #           dataloader's numba vox2pix pass can be dropped); a batch that brings tables is lifted from ITS tables,
    #           whatever origin / image-space transform they were built with;
    #   True    also when tables are present, provided the batch carries the float64 extrinsics the tables were made from
    #           (`T_velo_2_cam_f64`; float32 extrinsics move a few voxels by one pixel) -- the caller vouches that the tables
    #           are the plain vox2pix of that calibration;
    #   False   never.
    # OCCDEPTH_LIFT_PROJ = auto | 1 | 0.
    lift_in_kernel = {"1": True, "0": False}.get(os.environ.get("OCCDEPTH_LIFT_PROJ", "auto"), "auto")

    @staticmethod
    def _tables_absent(batch, key):
        """A batch brings no `key` entry (a voxel -> pixel table or a training target) when the key is missing, the list
        is empty, or every entry has zero elements (what a loader hooked by targets.defer_dataset_projection /
        defer_dataset_targets delivers)."""
        v = batch.get(key)
        if v is None:
            return True
        if torch.is_tensor(v):
            return v.numel() == 0
        return all(torch.is_tensor(t) and t.numel() == 0 for t in v)

    @staticmethod
    def _flip_mats(batch, E):
        """The batch's ida_mats as a (B, V, 4, 4) float32 tensor on E's device for the projection's flip flag
        (ida[b, v, 0, 0] < 0), or None without them.  Host matrices without a flip give None (nothing to read)."""
        ida = batch.get("ida_mats")
        if ida is None:
            return None
        t = torch.stack(list(ida)) if isinstance(ida, (list, tuple)) else ida
        if not t.is_cuda and not bool((t[..., 0, 0] < 0).any()):
            return None
        t = t.to(E.device, torch.float32).contiguous()
        if tuple(t.shape) != tuple(E.shape[:2]) + (4, 4):
            raise ValueError("ida_mats must be (batch, views, 4, 4) like the extrinsics, got %s" % (tuple(t.shape),))
        return t

    def _lift_calibration(self, batch, img, key):
        """(cam_E (B, V, 4, 4), cam_k (B, V, 3, 3)) float64 and ida (B, V, 4, 4) float32 (or None) device tensors for
        hip.lift_proj, or None when the in-kernel projection does not apply (NYU geometry, multi-point patterns, tables
        present and not vouched for)."""
        if not self.lift_in_kernel or self.dataset != "kitti" or "cam_k" not in batch:
            return None
        have_tables = not self._tables_absent(batch, key)
        if have_tables and (self.lift_in_kernel != True or "T_velo_2_cam_f64" not in batch):   # noqa: E712 ("auto" is truthy)
            return None
        ext = batch.get("T_velo_2_cam_f64", batch.get("T_velo_2_cam"))
        if ext is None:
            return None
        if have_tables and batch[key][0].shape[-2] != 1:
            return None                                          # multi-point pattern: table path
        dims = [int(d) // int(self.project_scale) for d in self.full_scene_size]
        if any(v & (v - 1) for v in dims[1:] + [int(r) for r in self.project_res]):
            return None                                          # the fused kernel indexes with shifts
        dev = img.device
        E = torch.stack([e.to(dev) for e in ext]).to(torch.float64)          # (B, V, 4, 4): 1-2 small launches
        k = torch.stack([c.to(dev) for c in batch["cam_k"]]).to(torch.float64)
        if E.shape[:2] != img.shape[:2] or E.shape[1] > 2 or k.shape[:2] != E.shape[:2]:
            return None
        return E.contiguous(), k.contiguous(), self._flip_mats(batch, E)

    def _forward_2d_to_3d(self, batch, x_rgb, img, bs, vox_origin):
        """eval: returns (Vox, depth_pred); training: ((B, C, X, Y, Z) tensor, depth_pred)."""
        key = "projected_pix_{}".format(self.project_scale)
        mkey = "fov_mask_{}".format(self.project_scale)
        scales = [int(s) for s in self.project_res]
        depth_vol = depth_pred = None
        if not needs_autograd(self):
            cam = self._lift_calibration(batch, img, key)
            if cam is not None:
                frustum = None
                if self.trans_2d_to_3d == "flosp_depth":
                    early = self.__dict__.pop("_early_depth", None)
                    if early is not None:                       # launched beside the decoder's fine levels: join here
                        torch.cuda.current_stream(img.device).wait_stream(self.__dict__["_depth_stream"])
                        frustum, depth_pred = early
                    else:
                        frustum, depth_pred = self._depth_volume(batch, x_rgb, vox_origin, defer_sample=True)
                feats = [[x_rgb[v]["1_" + str(s)] for v in range(len(x_rgb))] for s in scales]
                H, W = img.shape[-2:]
                vox = lift_scales_proj(feats, scales, cam[0], cam[1], self._kitti_origin(batch), 0.2 * self.project_scale, (W, H),
                                       self.projects[str(scales[0])].scene_size, self.project_scale, self.dataset,
                                       frustum=frustum, scale_const=100.0, ida=cam[2])
                return vox, depth_pred
        if self.trans_2d_to_3d == "flosp_depth":
            depth_vol, depth_pred = self._depth_volume(batch, x_rgb, vox_origin)
        if self._tables_absent(batch, key):
            # the loader shipped no tables (or the zero-size stubs of targets.defer_dataset_projection): build them here,
            # on the device, flip included -- in training too, and inside a captured step
            pix_all, fov_all = self.project_voxels_on_gpu(batch, img)
        else:
            pix_all = torch.stack([p.to(device) for p in batch[key]])
            fov_all = torch.stack([m.to(device) for m in batch[mkey]])
        if not needs_autograd(self):
            feats = [[x_rgb[v]["1_" + str(s)] for v in range(len(x_rgb))] for s in scales]
            flat = depth_vol.reshape(bs, -1).contiguous() if depth_vol is not None else None
            vox = lift_scales(feats, scales, pix_all, fov_all, self.projects[str(scales[0])].scene_size,
                              self.project_scale, self.dataset, depth_scale=flat, scale_const=100.0)
            return vox, depth_pred
        from .. import lift_autograd
        feats = [[x_rgb[v]["1_" + str(s)] for v in range(len(x_rgb))] for s in scales]
        if self.fused_lift and lift_autograd.usable(feats, pix_all) and self.dataset == "kitti":
            # training on the GPU, single-point patterns: the fused HIP lift with its one-launch backward
            # (the reference's per-sample / per-scale SFA calls and the `* depth * 100` in one differentiable op)
            x3ds = lift_autograd.lift_scales_autograd(feats, scales, pix_all, fov_all,
                                                      self.projects[str(scales[0])].scene_size, self.project_scale,
                                                      self.dataset, depth_scale=depth_vol, scale_const=100.0)
            return x3ds, depth_pred
        x3ds = []
        for i in range(bs):
            pix, fov = pix_all[i], fov_all[i]
            x3d = None
            for s in scales:
                stack = torch.stack([x_rgb[j]["1_" + str(s)] for j in range(len(x_rgb))], 1).to(device)
                part = self.projects[str(s)](stack[i], torch.div(pix, s, rounding_mode="floor"), fov)
                x3d = part if x3d is None else x3d + part
            x3ds.append(x3d)
        x3ds = torch.stack(x3ds)
        if depth_vol is not None:
            if self.dataset == "NYU":
                depth_vol = depth_vol.permute(0, 1, 2, 4, 3).contiguous()
            x3ds = x3ds * depth_vol * 100
        return x3ds, depth_pred

    # ---------------------------------------------------------------- evaluation report by region
    REPORT_PRESETS = {"kitti": ("full", "fov", "12.8m", "25.6m", "fov_12.8m", "fov_25.6m")}

    def enable_eval_report(self, regions="kitti", per_frame=False, mask_keys=()):
        """Count the test / validation steps into a second metric BY REGION beside the ordinary one, in one extra pass
        over the logits for all regions (loss/sscMetrics.py, hip.ssc_confusion_regions); `test_epoch_end` prints one block per region
        after the reference's report.  regions: the preset "kitti" -- `full`, `fov` (left camera), `12.8m` / `25.6m`
        (x in [0, r], |y| <= r / 2 metres from the sensor, all z) and their intersections with the FOV -- or a list of
        `Region`s with index boxes; their mask slots are filled from the batch entries named by `mask_keys` (lists of
        per-sample tensors or (B, ...) tensors).  per_frame keeps every frame's matrices (`report_metrics["test"].frame_stats()`)."""
        if isinstance(regions, str):
            if regions not in self.REPORT_PRESETS:
                raise ValueError("unknown eval report preset %r (have %s)" % (regions, sorted(self.REPORT_PRESETS)))
            if self.dataset != "kitti":
                raise NotImplementedError("the eval report preset %r is the SemanticKITTI geometry; a %s model takes a list "
                                          "of Region objects" % (regions, self.dataset))
        else:
            regions = tuple(regions)
        self.eval_report = {"regions": regions, "per_frame": bool(per_frame), "mask_keys": tuple(mask_keys)}
        self.report_metrics = {}
        return self

    def _report_regions(self, batch):
        from ..loss.sscMetrics import Region, metric_box
        regions = self.eval_report["regions"]
        if not isinstance(regions, str):
            return regions
        scale = -(-int(self.project_scale) // 2)           # the output scale of kitti_dataset.py:83
        grid = tuple(int(s) // scale for s in self.full_scene_size)
        origin = self._kitti_origin(batch)
        out = [Region("full"), Region("fov", fov=True)]
        for r in (12.8, 25.6):
            out.append(Region("%.1fm" % r, box=metric_box((0.0, r, -r / 2, r / 2), origin, 0.2 * scale, grid)))
        return out + [Region("fov_" + r.name, box=r.box, fov=True) for r in out[2:]]

    def _report_fov(self, batch, target):
        """The left camera's FOV at output scale: the batch's `fov_mask_1` when it is there and has the grid's size, else
        the calibration (float64 extrinsics when the batch carries them), from which the kernel computes the flag."""
        dev = target.device
        n = target[0].numel()
        fm = batch.get("fov_mask_1")
        if fm is not None and len(fm) == target.shape[0]:
            rows = []
            for t in fm:                              # (N,) / (N, 1), or the loader's (V, N, P): left view, pattern point 0
                t = torch.as_tensor(t).to(dev)
                if t.numel() == n:
                    rows.append(t.reshape(n))
                elif t.dim() > 1 and t[0].numel() >= n and t[0].numel() % n == 0:
                    rows.append(t[0].reshape(n, -1)[:, 0])
            if len(rows) == len(fm):
                return torch.stack(rows).contiguous()
        if self.dataset != "kitti":
            raise NotImplementedError("the FOV of a %s batch must come with it as fov_mask_1" % self.dataset)
        ext = batch.get("T_velo_2_cam_f64", batch["T_velo_2_cam"])
        E = torch.stack([e.to(dev) for e in ext]).to(torch.float64).contiguous()
        k = torch.stack([c.to(dev) for c in batch["cam_k"]]).to(torch.float64).contiguous()
        H, W = batch["img"].shape[-2:]
        return (E, k, self._kitti_origin(batch), 0.2 * -(-int(self.project_scale) // 2), (int(W), int(H)), (0,))

    def _report_count(self, step_type, batch, ssc_pred, target):
        from ..loss.sscMetrics import SSCMetrics
        metric = self.report_metrics.get(step_type)
        if metric is None:
            metric = self.report_metrics[step_type] = SSCMetrics(self.n_classes, regions=self._report_regions(batch),
                                                                 per_frame=self.eval_report["per_frame"])
        masks = []
        for key in self.eval_report["mask_keys"]:
            m = batch[key]
            masks.append(m if torch.is_tensor(m) else torch.stack([torch.as_tensor(t).to(target.device) for t in m]))
        fov = self._report_fov(batch, target) if any(r.fov for r in metric.regions) else None
        metric.add_batch_logits(ssc_pred, target, fov=fov, masks=masks)

    def _print_region_report(self, prefix):
        metric = self.report_metrics.get(prefix)
        if metric is None:
            return
        if self.metrics_allreduce and metric.region_hist is not None:
            from .. import shard
            shard.allreduce_confusion(metric.region_hist)
        classes = self.class_names
        for name, stats in metric.get_region_stats().items():
            print("{}[{}]======".format(prefix, name))
            print("Precision={:.4f}, Recall={:.4f}, IoU={:.4f}".format(
                stats["precision"] * 100, stats["recall"] * 100, stats["iou"] * 100))
            print("class IoU: {}, ".format(classes))
            print(" ".join(["{:.4f}, "] * len(classes)).format(*(stats["iou_ssc"] * 100).tolist()))
            print("mIoU={:.4f}".format(stats["iou_ssc_mean"] * 100))
        metric.reset()

    # ---------------------------------------------------------------- qualitative frames (render.py)
    RENDER_VOXEL_METRES = {"kitti": 0.2, "NYU": 0.08}       # full-resolution voxel of each dataset

    def enable_render(self, out_dir, every=1, views=("camera", "bev"), mode="class", overlay=False, max_frames=None):
        """Draw the prediction of every `every`-th test / validation batch on the GPU and write
        <out_dir>/<sequence>/<frame_id>_<view>.png (NYU: <out_dir>/<name>_<view>.png).  views: "camera" (the left camera's
        own view; overlay=True blends it over the input frame), "bev" (from above), "oblique" (third person).  mode
        "error" colours the prediction against the step's target.  Voxels outside the batch's `fov_mask_1` are dimmed.
        max_frames caps the frames written.  The pixels are the only device -> host transfer."""
        from .. import render
        views = tuple(views)
        bad = [v for v in views if v not in render.VIEW_NAMES]
        if bad or not views:
            raise ValueError("unknown render view(s) %s (have %s)" % (bad, render.VIEW_NAMES))
        if mode not in render.MODES:
            raise ValueError("unknown render mode %r (have %s)" % (mode, render.MODES))
        if int(every) < 1:
            raise ValueError("every must be >= 1, got %r" % (every,))
        self.render = {"out_dir": str(out_dir), "every": int(every), "views": views, "mode": mode, "overlay": bool(overlay),
                       "max_frames": None if max_frames is None else int(max_frames), "seen": 0, "written": 0,
                       "logged": False, "paths": []}
        return self

    def _render_views(self, batch, dims, img_hw, dev, names=None):
        """The ray generators of the enabled views (or of `names`) for this batch -> ([(18,) or (B, 18) tensors], [(h, w)])."""
        from .. import render
        vs = self.RENDER_VOXEL_METRES.get(self.dataset, 0.2) * float(self.full_scene_size[0]) / float(dims[0])

        def camera():
            origin = self._kitti_origin(batch) if self.dataset == "kitti" else None
            k, E, origin = render.batch_camera(batch, self.dataset, origin, dev)
            return render.camera_view(k, E, origin, vs), img_hw

        return render.standard_views(self.render["views"] if names is None else names, dims, dev, camera)

    def _render_names(self, batch, i, index):
        if "name" in batch:
            return "", str(batch["name"][i])
        seq = str(batch["sequence"][i]) if "sequence" in batch else "frames"
        return seq, str(batch["frame_id"][i]) if "frame_id" in batch else "%06d" % index

    def _render_logger(self):
        try:
            exp = getattr(self.logger, "experiment", None)
        except (AttributeError, RuntimeError):
            return None
        return exp if hasattr(exp, "add_image") else None

    def _render_step(self, step_type, batch, ssc_pred, target):
        from .. import hip, render
        st = self.render
        st["seen"] += 1
        if (st["seen"] - 1) % st["every"] or (st["max_frames"] is not None and st["written"] >= st["max_frames"]):
            return
        labels = hip.argmax_labels_u16(ssc_pred.detach())
        B = labels.shape[0]
        dims = tuple(int(d) for d in labels.shape[1:])
        dev = labels.device
        img = batch["img"]
        views, sizes = self._render_views(batch, dims, img.shape[-2:], dev)
        fov = self._report_fov(batch, target) if batch.get("fov_mask_1") is not None else None
        kw = {"fov": fov if torch.is_tensor(fov) else None, "mode": st["mode"], "n_classes": self.n_classes,
              "target": target if st["mode"] == "error" else None,
              "palette": self.dataset if self.dataset in ("kitti", "NYU") else None}
        images = [None] * len(views)
        rest = list(range(len(views)))
        if st["overlay"] and "camera" in st["views"]:
            c = st["views"].index("camera")
            mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
            std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
            frame = ((img[:, 0].to(dev).float() * std + mean).clamp(0, 1) * 255).to(torch.uint8)
            images[c] = render.render_labels(labels, [views[c]], sizes[c], background=frame.permute(0, 2, 3, 1)[:, None].contiguous(),
                                             **kw)[:, 0]
            rest.remove(c)
        if rest:
            for i, t in zip(rest, render.render_labels(labels, [views[i] for i in rest], [sizes[i] for i in rest], **kw)):
                images[i] = t
        # the only transfer: a few hundred KB per view into pinned memory, queued behind the step's kernels
        host = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True).copy_(t, non_blocking=True) for t in images]
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        for i in range(B):
            if st["max_frames"] is not None and st["written"] >= st["max_frames"]:
                break
            seq, frame_id = self._render_names(batch, i, st["written"])
            d = os.path.join(st["out_dir"], seq)
            os.makedirs(d, exist_ok=True)
            for name, h in zip(st["views"], host):
                st["paths"].append(render.write_png(os.path.join(d, "%s_%s.png" % (frame_id, name)), h[i].numpy()))
            st["written"] += 1
        exp = self._render_logger() if step_type == "val" and not st["logged"] else None
        if exp is not None:
            st["logged"] = True
            for name, h in zip(st["views"], host):
                exp.add_image("val_render/" + name, h[0].numpy(), getattr(self, "global_step", 0), dataformats="HWC")

    # ---------------------------------------------------------------- temporal fusion over a sequence (fuse.py)
    def enable_temporal_fusion(self, poses_root, window=4, decay=1.0, max_gap=None):
        """Fuse the prediction of every test / validation frame with up to `window - 1` earlier frames of its sequence
        (fuse.SequenceFuser: ego-motion from <poses_root>/<sequence>/poses.txt and calib.txt, weights decay^age, each
        earlier frame inside its own `fov_mask_1`) and count the fused labels into a SECOND metric beside the ordinary
        one: `val_fused/mIoU`, `val_fused/IoU` are logged and `test_epoch_end` prints a `test_fused======` block.  The
        ordinary metrics stay on the unfused logits.  The ring holds `window` frames of probabilities on the GPU (168 MB
        each at 256 x 256 x 32 x 20).  Frames must arrive in sequence order (no shuffling, one rank per sequence)."""
        if self.dataset != "kitti":
            raise NotImplementedError("temporal fusion reads SemanticKITTI poses and is wired for the SemanticKITTI geometry "
                                      "only; a %s model has no ego-motion to warp with" % self.dataset)
        if not poses_root:
            raise ValueError("temporal fusion needs the sequences directory (poses_root / OCCDEPTH_FUSE_POSES): "
                             "<root>/<sequence>/poses.txt and calib.txt")
        if not 1 <= int(window) <= 8:
            raise ValueError("window must be 1..8, got %r" % (window,))
        self.temporal_fusion = {"poses_root": str(poses_root), "window": int(window), "decay": float(decay),
                                "max_gap": None if max_gap is None else int(max_gap), "fuser": None, "poses": {}}
        self.fused_metrics = {}
        return self

    def _fuse_step(self, step_type, batch, ssc_pred, target):
        """Push every batch item, in order, through the sequence fuser and count the fused labels."""
        from .. import fuse
        from ..loss.sscMetrics import SSCMetrics
        st = self.temporal_fusion
        ssc_pred = ssc_pred.detach()
        B = ssc_pred.shape[0]
        dims = tuple(int(d) for d in ssc_pred.shape[2:])
        if st["fuser"] is None:
            vs = 0.2 * float(self.full_scene_size[0]) / float(dims[0])
            st["fuser"] = fuse.SequenceFuser(dims, self.n_classes, self._kitti_origin(batch), vs, window=st["window"],
                                             decay=st["decay"], max_gap=st["max_gap"])
        fov = self._report_fov(batch, target) if batch.get("fov_mask_1") is not None else None
        fov = fov if torch.is_tensor(fov) else None
        labels = []
        for i in range(B):
            seq = str(batch["sequence"][i])
            frame = int(batch["frame_id"][i])
            poses = st["poses"].get(seq)
            if poses is None:
                poses = st["poses"][seq] = fuse.read_kitti_poses(os.path.join(st["poses_root"], seq))
            if frame not in poses:
                raise KeyError("sequence %s has no pose for frame %d (%s)" % (seq, frame, os.path.join(st["poses_root"], seq, "poses.txt")))
            out = st["fuser"].push(ssc_pred[i].float(), poses[frame], key=(seq, frame), fov_mask=None if fov is None else fov[i])
            labels.append(out["y_pred"])
        metric = self.fused_metrics.get(step_type)
        if metric is None:
            metric = self.fused_metrics[step_type] = SSCMetrics(self.n_classes)
        labels = torch.stack(labels)
        metric.add_batch(labels, target)
        return labels

    # ---------------------------------------------------------------- RayIoU along sensor rays (ray_metric.py)
    def enable_ray_metrics(self, thresholds_m=(1, 2, 4), origins=1, origin_step=5, poses_root=None, unknown="drop",
                           **direction_kwargs):
        """Score every test / validation frame along sensor rays as well (ray_metric.RayMetrics, K35: RayIoU of "Fully
        Sparse 3D Occupancy Prediction", Liu et al., 2024).  The rays of ray_metric.lidar_directions(**direction_kwargs)
        (a 64-beam stand-in fan, not a sensor's calibration table) are cast from the velodyne origin through the arg-max of
        the unfused logits and through the target in one launch per step; a ray is a true positive of class c at
        threshold tau when both hit class c and the depths differ by less than tau.  `val_ray/RayIoU`, `val_ray/RayIoU@<tau>`
        per threshold and `val_ray/RayIoU_geo` (class-agnostic, mean over the thresholds) are logged and `test_epoch_end`
        prints a `test_ray======` block with the per-class table and the ray tallies; with temporal fusion on its fused
        labels are scored into a second metric (`val_fused_ray/*`, `test_fused_ray======`).  The ordinary metrics are
        untouched.  unknown: "drop" (a ray that meets a target voxel 255 before its target hit is left out) or "pass"
        (255 is seen through).  origins > 1: the sensor positions of the frames t, t + origin_step, ... (up to `origins`,
        those inside the grid; ray_metric.trajectory_origins) are ray origins too, which scores surfaces hidden from the
        current position; that needs the ego-motion, <poses_root>/<sequence>/poses.txt and calib.txt.  With
        metrics_allreduce the counters are summed over the ranks before the statistics.  No RayIoU of a trained model is
        measured (no checkpoint and no dataset where this was built)."""
        if self.dataset != "kitti":
            raise NotImplementedError("ray metrics cast a lidar's rays from the velodyne origin and are wired for the "
                                      "SemanticKITTI geometry only; a %s model has no sensor origin to cast from" % self.dataset)
        if int(origins) < 1 or int(origin_step) < 1:
            raise ValueError("origins and origin_step must be >= 1, got %r, %r" % (origins, origin_step))
        if int(origins) > 1 and not poses_root:
            raise ValueError("ray metrics from more than one origin need the sequences directory (poses_root / "
                             "OCCDEPTH_RAY_POSES, or OCCDEPTH_FUSE_POSES): <root>/<sequence>/poses.txt and calib.txt")
        if unknown not in ("drop", "pass"):
            raise ValueError("unknown is 'drop' or 'pass' (OCCDEPTH_RAY_UNKNOWN), got %r" % (unknown,))
        thresholds_m = tuple(float(t) for t in thresholds_m)
        if not 1 <= len(thresholds_m) <= 4 or any(not t > 0.0 for t in thresholds_m):
            raise ValueError("1..4 positive thresholds in metres, got %r" % (thresholds_m,))
        self.ray_metrics = {"thresholds_m": thresholds_m, "origins": int(origins), "origin_step": int(origin_step),
                            "poses_root": str(poses_root) if poses_root else None, "unknown": unknown,
                            "directions": dict(direction_kwargs), "dirs": None, "poses": {}, "metrics": {}, "fused": {}}
        return self

    def _ray_step(self, step_type, batch, ssc_pred, target, fused_labels=None, pred_labels=None):
        """Cast the rays through every batch item's arg-max labels (and the fused labels, if any) and its target.
        pred_labels: the arg-max of ssc_pred when the caller already has it."""
        from .. import hip, ray_metric
        st = self.ray_metrics
        ssc_pred = ssc_pred.detach()
        B = ssc_pred.shape[0]
        dims = tuple(int(d) for d in ssc_pred.shape[2:])
        vs = 0.2 * float(self.full_scene_size[0]) / float(dims[0])
        origin = self._kitti_origin(batch)
        if st["dirs"] is None:
            st["dirs"] = ray_metric.lidar_directions(**st["directions"])
        if st["origins"] > 1:                                            # every pose first: a refusal launches nothing
            from .. import fuse
            origins = []
            for i in range(B):
                seq = str(batch["sequence"][i])
                frame = int(batch["frame_id"][i])
                poses = st["poses"].get(seq)
                if poses is None:
                    poses = st["poses"][seq] = fuse.read_kitti_poses(os.path.join(st["poses_root"], seq))
                if frame not in poses:
                    raise KeyError("sequence %s has no pose for frame %d (%s)" % (seq, frame, os.path.join(st["poses_root"], seq, "poses.txt")))
                origins.append(ray_metric.trajectory_origins(poses, frame, st["origins"], st["origin_step"], origin, vs, dims))
        else:
            origins = [ray_metric.sensor_origin(origin, vs)[None]] * B
        # (B, X, Y, Z) uint16 bits, the unfused logits
        pred = hip.argmax_labels_u16(ssc_pred.float()) if pred_labels is None else pred_labels
        gt = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).reshape((B,) + dims)
        for store, labels in ((st["metrics"], pred), (st["fused"], fused_labels)):
            if labels is None:
                continue
            metric = store.get(step_type)
            if metric is None:
                metric = store[step_type] = ray_metric.RayMetrics(self.n_classes, vs, st["dirs"], st["thresholds_m"], st["unknown"])
            if len(set(len(o) for o in origins)) == 1:                   # one launch for the batch
                metric.add_batch(labels, gt, torch.stack(list(origins)))
            else:                                                        # frames kept different numbers of origins
                for i in range(B):
                    metric.add_batch(labels[i:i + 1], gt[i:i + 1], origins[i][None])

    def _ray_epoch_end(self, step_type):
        """-> [(prefix, statistics)] of the ray metrics of `step_type` that counted something, reset."""
        out = []
        for name, store in (("ray", self.ray_metrics["metrics"]), ("fused_ray", self.ray_metrics["fused"])):
            metric = store.get(step_type)
            if metric is None:
                continue
            if self.metrics_allreduce:
                metric.allreduce_()
            out.append(("%s_%s" % (step_type, name), metric.get_stats()))
            metric.reset()
        return out

    # ---------------------------------------------------------------- distance-tolerant scores (dist_metric.py)
    def enable_distance_metrics(self, thresholds_m=(0.2, 0.4, 0.8), max_d2=1024, fov_only=False):
        """Score every test / validation frame by distance as well (dist_metric.DistanceMetrics, K37): for every predicted
        occupied voxel the distance to the nearest true one and the other way round, class-agnostic and per class, from
        the exact distance transform of both label volumes on the GPU.  The arg-max of the unfused logits is scored against
        the target in one call per step; `val_dist/F_geo@<tau>` and `val_dist/F_sem@<tau>` per threshold (metres),
        `val_dist/CD_geo` and `val_dist/CD_sem` (the Chamfer distance in metres, truncated at voxel_size * sqrt(max_d2 + 1)
        per side) are logged and `test_epoch_end` prints a `test_dist======` block with the per-class table; with temporal
        fusion on its fused labels are scored into a second metric (`val_fused_dist/*`, `test_fused_dist======`).  The
        ordinary metrics are untouched.  Target voxels 255 are no queries (their neighbours' predictions still serve as
        seeds); fov_only: only voxels inside the batch's full-scale FOV mask (`fov_mask_1`) are queries.  The metric
        needs the grid alone, so it works for every dataset; the voxel size is the dataset's.  With metrics_allreduce the
        counters are summed over the ranks before the statistics.  No score of a trained model is measured (no
        checkpoint and no dataset where this was built)."""
        thresholds_m = tuple(float(t) for t in thresholds_m)
        if not thresholds_m or any(not t > 0.0 for t in thresholds_m):
            raise ValueError("at least one positive threshold in metres, got %r" % (thresholds_m,))
        if not 1 <= int(max_d2) <= 65534:
            raise ValueError("max_d2 must be 1..65534, got %r" % (max_d2,))
        self.dist_metrics = {"thresholds_m": thresholds_m, "max_d2": int(max_d2), "fov_only": bool(fov_only),
                             "metrics": {}, "fused": {}}
        return self

    def _dist_step(self, step_type, batch, ssc_pred, target, fused_labels=None, pred_labels=None):
        """Add the batch's arg-max labels (and the fused labels, if any) against its target to the distance histograms.
        pred_labels: the arg-max of ssc_pred when the caller already has it."""
        from .. import dist_metric, hip
        st = self.dist_metrics
        ssc_pred = ssc_pred.detach()
        B = ssc_pred.shape[0]
        dims = tuple(int(d) for d in ssc_pred.shape[2:])
        vs = OccDepth.RENDER_VOXEL_METRES.get(self.dataset, 0.2) * float(self.full_scene_size[0]) / float(dims[0])
        mask = None
        if st["fov_only"]:
            mask = self._report_fov(batch, target) if batch.get("fov_mask_1") is not None else None
            if not torch.is_tensor(mask):
                raise ValueError("fov_only distance metrics need the batch's full-scale FOV mask (fov_mask_1)")
            mask = mask.reshape((B,) + dims)
        pred = hip.argmax_labels_u16(ssc_pred.float()) if pred_labels is None else pred_labels
        gt = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).reshape((B,) + dims)
        for store, labels in ((st["metrics"], pred), (st["fused"], fused_labels)):
            if labels is None:
                continue
            metric = store.get(step_type)
            if metric is None:
                metric = store[step_type] = dist_metric.DistanceMetrics(self.n_classes, vs, st["thresholds_m"], st["max_d2"])
            metric.add_batch(labels, gt, mask)

    def _dist_epoch_end(self, step_type):
        """-> [(prefix, statistics)] of the distance metrics of `step_type` that counted something, reset."""
        out = []
        for name, store in (("dist", self.dist_metrics["metrics"]), ("fused_dist", self.dist_metrics["fused"])):
            metric = store.get(step_type)
            if metric is None:
                continue
            if self.metrics_allreduce:
                metric.allreduce_()
            out.append(("%s_%s" % (step_type, name), metric.get_stats()))
            metric.reset()
        return out

    # ---------------------------------------------------------------- panoptic quality (panoptic.py)
    def enable_panoptic_metrics(self, connectivity=26, min_pred_voxels=1, things=None, stuff=None, fov_only=False):
        """Score every test / validation frame by objects as well (panoptic.PanopticMetrics, K40): the connected components
        of the arg-max of the unfused logits -- per `things` class, under `connectivity` 6 or 26, components of fewer than
        min_pred_voxels voxels removed first -- and one segment per `stuff` class are matched to the segments of the target
        at IoU > 1/2.  `val_pan/PQ`, `PQ_things`, `PQ_stuff`, `SQ`, `RQ` and `PQ_dagger` are logged and `test_epoch_end`
        prints a `test_pan======` block with the per-class table; with temporal fusion on its fused labels are scored
        into a second metric (`val_fused_pan/*`, `test_fused_pan======`).  The ordinary metrics are untouched.  The
        target's "instances" are the connected components of the target (the completion volumes carry no instance
        annotation).  things / stuff: None = the dataset's defaults (panoptic.default_classes).  Target voxels 255 do
        not count; fov_only: only voxels inside the batch's full-scale FOV mask (`fov_mask_1`) count.  With
        metrics_allreduce the counters are summed over the ranks before the statistics.  No PQ of a trained model is
        measured (no checkpoint and no dataset where this was built)."""
        if int(connectivity) not in (6, 26):
            raise ValueError("connectivity must be 6 or 26, got %r" % (connectivity,))
        if int(min_pred_voxels) < 1:
            raise ValueError("min_pred_voxels must be >= 1, got %r" % (min_pred_voxels,))
        if things is None or stuff is None:
            from ..panoptic import default_classes
            d_things, d_stuff = default_classes(self.dataset)
            things, stuff = (d_things if things is None else things), (d_stuff if stuff is None else stuff)
        things, stuff = tuple(int(c) for c in things), tuple(int(c) for c in stuff)
        if set(things) & set(stuff):
            raise ValueError("things %r and stuff %r overlap" % (things, stuff))
        self.panoptic_metrics = {"connectivity": int(connectivity), "min_pred_voxels": int(min_pred_voxels), "things": things,
                                 "stuff": stuff, "fov_only": bool(fov_only), "metrics": {}, "fused": {}}
        return self

    def _pan_step(self, step_type, batch, ssc_pred, target, fused_labels=None, pred_labels=None):
        """Add the batch's arg-max labels (and the fused labels, if any) against its target to the panoptic counters."""
        from .. import hip, panoptic
        st = self.panoptic_metrics
        ssc_pred = ssc_pred.detach()
        B = ssc_pred.shape[0]
        dims = tuple(int(d) for d in ssc_pred.shape[2:])
        mask = None
        if st["fov_only"]:
            mask = self._report_fov(batch, target) if batch.get("fov_mask_1") is not None else None
            if not torch.is_tensor(mask):
                raise ValueError("fov_only panoptic metrics need the batch's full-scale FOV mask (fov_mask_1)")
            mask = mask.reshape((B,) + dims)
        pred = hip.argmax_labels_u16(ssc_pred.float()) if pred_labels is None else pred_labels
        gt = (target if target.dtype == torch.uint8 else target.to(torch.uint8)).reshape((B,) + dims)
        for store, labels in ((st["metrics"], pred), (st["fused"], fused_labels)):
            if labels is None:
                continue
            metric = store.get(step_type)
            if metric is None:
                metric = store[step_type] = panoptic.PanopticMetrics(self.n_classes, st["things"], st["stuff"],
                                                                     st["connectivity"], st["min_pred_voxels"])
            metric.add_batch(labels, gt, mask)

    def _pan_epoch_end(self, step_type):
        """-> [(prefix, statistics)] of the panoptic metrics of `step_type` that counted something, reset."""
        out = []
        for name, store in (("pan", self.panoptic_metrics["metrics"]), ("fused_pan", self.panoptic_metrics["fused"])):
            metric = store.get(step_type)
            if metric is None:
                continue
            if self.metrics_allreduce:
                metric.allreduce_()
            out.append(("%s_%s" % (step_type, name), metric.get_stats()))
            metric.reset()
        return out

    # ---------------------------------------------------------------- sequence-level semantic map (semantic_map.py)
    def enable_semantic_map(self, out_dir, poses_root, min_obs=1, views=(), frames=False, submission_dir=None,
                            exclude_self=False, max_frames=1024, gather=True, save_maps=False, visibility=None, mesh=False):
        """Vote every test / validation frame into a world-frame voxel map of its sequence (semantic_map.SemanticMap:
        ego-motion from <poses_root>/<sequence>/poses.txt and calib.txt): the arg-max of the unfused logits into the
        prediction map and the frame's target into the ground-truth map, both inside the frame's `fov_mask_1` when the
        batch has one.  At the end of the epoch every sequence's maps are written to <out_dir>/<step>_<sequence>_pred.ply
        and _gt.ply (voxels with at least `min_obs` votes), the prediction maps are scored against the ground-truth maps
        where both were observed -- `val_map/mIoU`, `val_map/IoU` are logged, `test_epoch_end` prints a `test_map======`
        block -- and the maps are released.  Votes commute, so frames may arrive in any order and on any rank: with gather
        (the default; OCCDEPTH_MAP_GATHER=0 or gather=False turns it off) and a torch.distributed process group of more
        than one rank, the epoch end first sums every sequence's maps over the ranks (semantic_map.merge_over_ranks, K33:
        the ranks agree on the (step, sequence) keys, a rank without a frame of a sequence brings an empty pair, the
        prediction map and then the ground-truth map of every key in sorted order), so every rank holds the map of all
        frames.  Then PLYs, PNGs and .occmap files are written by rank 0 alone; `val_map/*` is computed on every rank
        from the identical maps and never summed over ranks, not even with metrics_allreduce; `val_mapped/*` counts each
        rank's own kept frames against the merged prediction map and follows the ordinary metric's metrics_allreduce
        rule; every rank writes the submission files of the frames it kept (their names differ by frame).  A frame that
        voted on more than one rank (DistributedSampler pads by repeating frames) votes twice, as the ordinary metric
        counts it twice: one warning gives their number.  With one rank, or gather off, every rank does what a single
        process does.  save_maps (OCCDEPTH_MAP_SAVE=1): before the maps are released their vote counters are kept as
        <out_dir>/<step>_<sequence>_{pred,gt}.occmap (SemanticMap.save; SemanticMap.load and merge resume from them).
        Memory: 163840 bytes per 16^3 brick and map at 20 classes.  views: any of "bev", "oblique" -- before the
        maps are released every sequence is also drawn (render.render_map on semantic_map.MapVolume(pred, gt, min_obs))
        to <out_dir>/<step>_<sequence>_{pred,gt,err}_{view}.png; () draws nothing and imports nothing more.

        frames (or a submission_dir, which switches it on): the map is also read back into every frame (K32,
        SemanticMap.sample).  Every frame's prediction (uint8), target (uint8), the FOV mask it voted with, its pose,
        sequence and frame id are kept on the GPU until the epoch ends -- three bytes per voxel, 6.3 MB per frame at
        256 x 256 x 32, about 5 GB for the 815 validation frames of sequence 08; more than `max_frames` kept frames
        raise instead of running the allocator dry.  Before the maps are released each kept frame is sampled from its
        sequence's PREDICTION map (own = its prediction, own_mask = its mask, min_obs, keep_own; exclude_self takes the
        frame's own vote out) and counted against its target into a third metric: `val_mapped/mIoU`, `val_mapped/IoU`
        are logged and `test_epoch_end` prints a `test_mapped======` block.  With submission_dir the mapped labels are
        written as <submission_dir>/sequences/<seq>/predictions/<frame>.label (output.write_kitti_submission_labels).
        Off: nothing more is kept, imported or launched.  The effect on any score is not measured.

        visibility = (w_visible, w_hidden) (OCCDEPTH_MAP_VISIBILITY=<w_vis>,<w_hid>; integers, 1 <= w_visible <= 255,
        0 <= w_hidden <= 255): occlusion-aware votes.  The pixel rays of the batch's left camera (`cam_k`,
        `T_velo_2_cam`, the size of `img`) are cast through every PREDICTED volume (visibility.visible_voxels, K34); a
        voxel a ray reaches, up to and including the first occupied one, votes into the prediction map with w_visible,
        every other voxel inside the FOV mask with w_hidden, so a frame that only guessed a voxel no longer outvotes one
        that saw it.  The ground-truth map is unchanged.  Kept frames hold that weight volume where they held the mask
        (the same bytes), the read-back retracts it under exclude_self, and min_obs counts vote units.  None (the
        default): nothing more is imported or launched.  The effect on mIoU is not measured.

        mesh (OCCDEPTH_MAP_MESH=1): before the maps are released -- after the exchange over the ranks, by rank 0 alone --
        every sequence's maps are also written as closed surface meshes, <out_dir>/<step>_<sequence>_{pred,gt}_mesh.ply
        (mesh.mesh_map with min_obs, K39: one quad per exposed voxel face, every lattice corner once; mesh.write_mesh_ply).
        False (the default): mesh.py is not imported and nothing more is allocated or launched."""
        if visibility is not None:
            if len(tuple(visibility)) != 2:
                raise ValueError("visibility is (w_visible, w_hidden) (OCCDEPTH_MAP_VISIBILITY=<w_vis>,<w_hid>), got %r" % (visibility,))
            from ..visibility import check_weights
            visibility = check_weights(*visibility)
        if self.dataset != "kitti":
            raise NotImplementedError("the semantic map reads SemanticKITTI poses and is wired for the SemanticKITTI geometry "
                                      "only; a %s model has no ego-motion to lay its frames out with" % self.dataset)
        if not poses_root:
            raise ValueError("the semantic map needs the sequences directory (poses_root / OCCDEPTH_MAP_POSES, or "
                             "OCCDEPTH_FUSE_POSES): <root>/<sequence>/poses.txt and calib.txt")
        if not out_dir:
            raise ValueError("the semantic map needs a directory to write its PLY files to (out_dir / OCCDEPTH_MAP_DIR)")
        if int(min_obs) < 1:
            raise ValueError("min_obs must be >= 1, got %r" % (min_obs,))
        views = tuple(str(v) for v in views)
        if any(v not in ("bev", "oblique") for v in views):
            raise ValueError("a map view is 'bev' or 'oblique' (views / OCCDEPTH_MAP_VIEWS), got %r" % (views,))
        if int(max_frames) < 1:
            raise ValueError("max_frames must be >= 1, got %r" % (max_frames,))
        self.semantic_map = {"out_dir": str(out_dir), "poses_root": str(poses_root), "min_obs": int(min_obs),
                             "maps": {}, "poses": {}, "paths": [], "views": views,
                             "frames": bool(frames) or bool(submission_dir), "submission_dir": str(submission_dir) if submission_dir else None,
                             "exclude_self": bool(exclude_self), "max_frames": int(max_frames), "kept": {}, "mapped_stats": {},
                             "gather": bool(gather), "save_maps": bool(save_maps), "seen": {}, "visibility": visibility,
                             "mesh": bool(mesh)}
        return self

    def _map_step(self, step_type, batch, ssc_pred, target):
        """Every batch item votes into its sequence's prediction map and ground-truth map."""
        from .. import fuse, hip, semantic_map
        st = self.semantic_map
        ssc_pred = ssc_pred.detach()
        B = ssc_pred.shape[0]
        dims = tuple(int(d) for d in ssc_pred.shape[2:])
        vs = 0.2 * float(self.full_scene_size[0]) / float(dims[0])
        origin = self._kitti_origin(batch)
        fov = self._report_fov(batch, target) if batch.get("fov_mask_1") is not None else None
        fov = fov if torch.is_tensor(fov) else None
        items = []
        for i in range(B):                                               # every pose first: a refusal launches nothing
            seq = str(batch["sequence"][i])
            frame = int(batch["frame_id"][i])
            poses = st["poses"].get(seq)
            if poses is None:
                poses = st["poses"][seq] = fuse.read_kitti_poses(os.path.join(st["poses_root"], seq))
            if frame not in poses:
                raise KeyError("sequence %s has no pose for frame %d (%s)" % (seq, frame, os.path.join(st["poses_root"], seq, "poses.txt")))
            items.append((seq, poses[frame]))
        if st.get("frames"):
            kept = sum(len(v) for v in st["kept"].values())
            if kept + B > st["max_frames"]:
                raise RuntimeError("the map read-back would keep %d frames on the GPU, max_frames = %d (%.1f MB per frame: "
                                   "prediction, target and mask); raise max_frames or evaluate fewer frames per epoch"
                                   % (kept + B, st["max_frames"], 3e-6 * dims[0] * dims[1] * dims[2]))
        pred = hip.argmax_labels_u16(ssc_pred.float())                   # (B, X, Y, Z) uint16 bits, the unfused logits
        gt = target if target.dtype == torch.uint8 else target.to(torch.uint8)
        weights = st.get("visibility")
        if weights:                                                      # the left camera's pixel rays, one view per item
            from .. import render, visibility
            missing = [k for k in ("cam_k", "T_velo_2_cam", "img") if k not in batch]
            if missing:
                raise KeyError("occlusion-aware map votes need the camera of every frame: the batch has no %s" % ", ".join(missing))
            cam_k, cam_E, _ = render.batch_camera(batch, self.dataset, origin, pred.device)
            rays, rays_hw = visibility.camera_rays(cam_k, cam_E, origin, vs, tuple(batch["img"].shape[-2:]))
        for i, (seq, pose) in enumerate(items):
            pair = st["maps"].get((step_type, seq))
            if pair is None:
                pair = st["maps"][(step_type, seq)] = tuple(semantic_map.SemanticMap(self.n_classes, vs, origin, dims)
                                                            for _ in range(2))
            mask = None if fov is None else fov[i]
            weight = None
            if weights:
                weight = visibility.vote_weights(visibility.visible_voxels(pred[i], rays[i], rays_hw), mask, *weights)
                pair[0].integrate(pred[i], pose, weight=weight)
            else:
                pair[0].integrate(pred[i], pose, mask=mask)
            pair[1].integrate(gt[i].reshape(dims), pose, mask=mask)
            st.setdefault("seen", {}).setdefault(step_type, []).append((seq, int(batch["frame_id"][i])))
            if st.get("frames"):                                         # the weight volume takes the mask's place: the same bytes
                voted = weight if weights else (None if mask is None else mask != 0)
                st["kept"].setdefault((step_type, seq), []).append(      # copies: the batch's tensors are not held on to
                    (pred[i].to(torch.uint8), gt[i].reshape(dims).clone(), voted, pose, str(batch["frame_id"][i])))

    def _map_epoch_end(self, step_type):
        """Write and score the maps of `step_type`, release them; -> the statistics over its sequences, or None."""
        from .. import render, semantic_map
        from ..loss.sscMetrics import SSCMetrics
        st = self.semantic_map
        mine = sorted(key for key in st["maps"] if key[0] == step_type)
        seen = st.setdefault("seen", {}).pop(step_type, [])
        gathered, writer = False, True
        if st.get("gather", True):
            import torch.distributed as dist
            gathered = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if gathered:
            # every rank issues the same collectives in the same order: the keys, then per key the two maps
            said = [None] * dist.get_world_size()
            shapes = {key: (st["maps"][key][0].voxel_size, st["maps"][key][0].vox_origin, st["maps"][key][0].dims) for key in mine}
            dist.all_gather_object(said, (shapes, sorted(set(seen))))
            writer = dist.get_rank() == 0
            held = {}
            for shapes_r, seen_r in said:
                for frame in seen_r:
                    held[frame] = held.get(frame, 0) + 1
            twice = sum(1 for n in held.values() if n > 1)
            if twice:
                import warnings
                warnings.warn("occdepth_amd: %d frame(s) of the %s epoch voted on more than one rank (the sampler pads by "
                              "repeating frames): they vote twice, as the ordinary metric counts them twice" % (twice, step_type))
            known = {}
            for shapes_r, _ in said:
                known.update(shapes_r)
            mine = sorted(known)
            for key in mine:
                if key not in st["maps"]:
                    vs, origin, dims = known[key]
                    st["maps"][key] = tuple(semantic_map.SemanticMap(self.n_classes, vs, origin, dims) for _ in range(2))
                for m in st["maps"][key]:
                    semantic_map.merge_over_ranks(m)
        if not mine:
            return None
        os.makedirs(st["out_dir"], exist_ok=True)
        metric = SSCMetrics(self.n_classes)
        colours = render.palette("kitti" if self.n_classes == 20 else int(self.n_classes))
        mapped = SSCMetrics(self.n_classes) if st.get("frames") else None
        for key in mine:
            pair = st["maps"].pop(key)
            for own, gt, own_mask, pose, frame_id in (st["kept"].pop(key, ()) if mapped is not None else ()):
                voted = {"own_weight": own_mask} if st.get("visibility") else {"own_mask": own_mask}
                labels, _ = pair[0].sample(pose, own=own, min_obs=st["min_obs"], exclude_self=st["exclude_self"], keep_own=True,
                                           **voted)
                mapped.add_batch(labels[None], gt[None])
                if st["submission_dir"]:
                    from .. import output
                    st["paths"].append(output.write_kitti_submission_labels(labels, key[1], frame_id, st["submission_dir"]))
            for m, name in zip(pair, ("pred", "gt")) if writer else ():
                coords, labels, n_obs = m.extract(min_obs=st["min_obs"])
                path = os.path.join(st["out_dir"], "%s_%s_%s.ply" % (step_type, key[1], name))
                st["paths"].append(semantic_map.write_ply(path, coords, labels, n_obs, m.voxel_size, colours))
                if st.get("save_maps"):
                    st["paths"].append(m.save(os.path.join(st["out_dir"], "%s_%s_%s.occmap" % (step_type, key[1], name))))
            if st.get("mesh") and writer:
                from .. import mesh as surface
                for part, name in zip(surface.mesh_map(pair[0], pair[1], st["min_obs"]), ("pred", "gt")):
                    path = os.path.join(st["out_dir"], "%s_%s_%s_mesh.ply" % (step_type, key[1], name))
                    st["paths"].append(surface.write_mesh_ply(path, part, colours))
            semantic_map.map_confusion(pair[0], pair[1], metric)
            if st.get("views") and writer:
                volume = semantic_map.MapVolume(pair[0], pair[1], st["min_obs"])
                prefix = os.path.join(st["out_dir"], "%s_%s" % (step_type, key[1]))
                st["paths"] += render.write_map_pictures(volume, prefix, st["views"], palette=colours)
            for m in pair:
                m.release()
        if mapped is not None:
            st["mapped_stats"][step_type] = self._epoch_stats(mapped)
        # after the exchange every rank counted the same maps: their statistics are never summed over the ranks
        return metric.get_stats() if gathered else self._epoch_stats(metric)

    def _kitti_origin(self, batch=None):
        """SemanticKITTI voxel origin (kitti_dataset.py:82: vox_origin = (0, -25.6, -2) for the 51.2 m wide scene): the grid
        is centred on the sensor in y, whatever the scene width of a reduced test config.  A batch that carries its own
        `vox_origin` (host or device tensor / array / tuple; the reference's kitti collate does not) overrides it."""
        vo = None if batch is None else batch.get("vox_origin")
        if vo is not None:
            v = vo if torch.is_tensor(vo) else torch.as_tensor(vo[0] if isinstance(vo, (list, tuple)) and torch.is_tensor(vo[0]) else vo)
            if not v.is_cuda:
                return tuple(float(x) for x in v.reshape(-1, 3)[0])
            # A device tensor (Lightning's transfer_batch_to_device moves every batch tensor): the origin is a constant of
            # the dataset, so it is read back ONCE per model (one host sync, outside any graph capture) and the host copy
            # is reused for every later batch that brings a device `vox_origin` -- never silently ignored.
            cached = getattr(self, "_vox_origin_from_device", None)
            if cached is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("batch['vox_origin'] is a device tensor first seen during graph capture; run one eager "
                                       "forward first or pass it as a host tensor")
                cached = tuple(float(x) for x in v.detach().reshape(-1, 3)[0].cpu())
                self._vox_origin_from_device = cached
                default = (0.0, -0.1 * float(self.full_scene_size[1]), -2.0)
                if cached != default:
                    import warnings
                    warnings.warn("occdepth_amd: using the batch's device vox_origin %s (read once, assumed constant over "
                                  "the dataset) instead of the SemanticKITTI default %s" % (cached, default))
            return cached
        return (0.0, -0.1 * float(self.full_scene_size[1]), -2.0)

    def project_voxels_on_gpu(self, batch, img):
        """when the batch carries no `projected_pix_{s}` / `fov_mask_{s}` (the dataloader's
        numba `vox2pix`, kitti_dataset.py:253-273), compute them on the GPU from the calibration (SemanticKITTI geometry:
        vox_origin (0, -25.6, -2), 0.2 m voxels x project_scale, pattern_id 0) in ONE launch (hip.vox2pix): device
        calibration, no host sync, capture-safe.  Views flipped by the loader (ida_mats[..., 0, 0] < 0) get the flipped
        tables of kitti_dataset.py:384-390.  -> (B, V, N, 1, 2) int64, (B, V, N, 1) bool."""
        from .. import hip
        if self.dataset != "kitti":
            raise NotImplementedError("on-GPU voxel projection is wired for the SemanticKITTI geometry only; a %s batch "
                                      "must bring projected_pix_%s / fov_mask_%s" % (self.dataset, self.project_scale,
                                                                                    self.project_scale))
        if not img.is_cuda:
            raise RuntimeError("the voxel -> pixel tables are built on the GPU only (occd_vox2pix); a CPU batch must bring "
                               "projected_pix_%s / fov_mask_%s" % (self.project_scale, self.project_scale))
        ps = self.project_scale
        dims = tuple(int(s) // ps for s in self.full_scene_size)
        H, W = img.shape[-2:]
        dev = img.device
        # the dataloader projects with the calibration file's float64 extrinsics; the batch only carries their float32
        # copy.  `T_velo_2_cam_f64`, when present, reproduces the dataloader's tables bit for bit.
        ext = batch.get("T_velo_2_cam_f64", batch["T_velo_2_cam"])
        E = torch.stack([e.to(dev) for e in ext]).to(torch.float64).contiguous()
        k = torch.stack([c.to(dev) for c in batch["cam_k"]]).to(torch.float64).contiguous()
        return hip.vox2pix(E, k, self._flip_mats(batch, E), self._kitti_origin(batch), 0.2 * ps, dims, (int(W), int(H)))

    # ---------------------------------------------------------------- stereo depth target on the GPU
    def enable_stereo_depth(self, max_disp=192, p1=10, p2=120, uniqueness=95, mean=None, std=None):
        """Build the depth target of `use_stereo_depth_gt` in the step, from the batch's rectified image pair and its
        calibration (stereo.stereo_depth: census, four-path SGM, uniqueness / left-right / inner checks, sub-pixel fit,
        depth = f B / disparity), for every batch that brings no `gt_depth` (key missing or zero elements: what a loader
        hooked by targets.defer_dataset_stereo_depth delivers).  A batch that brings `gt_depth` is used as it is; the batch
        is never modified; "test" steps build nothing.  Works eagerly and inside the captured training step (no host
        read, the workspace is allocated per call).  max_disp: a multiple of 64 in 64..256; mean / std: the loader's
        normalisation (ImageNet's by default).  The same switch from the environment: OCCDEPTH_GPU_STEREO=1.

        What is matched: `img` (B, 2, 3, H, W), view 0 taken to be the LEFT camera of a rectified pair, turned back into
        8-bit gray.  The loader jitters colour per view independently (kitti_dataset.py:374): census depends only on the
        local order of gray values, so brightness and contrast changes are harmless; matching quality under saturation or
        hue jitter is not claimed.  A batch key `img_gray_u8` (B, 2, H, W) uint8 -- the un-jittered pair -- is matched
        instead of `img` when present.  Frames the loader mirrored (ida_mats[b, 0, 0, 0] < 0) are matched towards x + d."""
        from .. import stereo
        max_disp = int(max_disp)
        if max_disp % 64 or not 64 <= max_disp <= 256:
            raise ValueError("enable_stereo_depth: max_disp must be a multiple of 64 in 64..256, got %d" % max_disp)
        if not 0 <= int(p1) <= int(p2) <= 193 or not 1 <= int(uniqueness) <= 100:
            raise ValueError("enable_stereo_depth: needs 0 <= p1 <= p2 <= 193 and uniqueness in 1..100, got p1=%s p2=%s "
                             "uniqueness=%s" % (p1, p2, uniqueness))
        self.gpu_stereo = dict(max_disp=max_disp, p1=int(p1), p2=int(p2), uniqueness=int(uniqueness),
                               mean=tuple(mean) if mean is not None else stereo.IMAGENET_MEAN,
                               std=tuple(std) if std is not None else stereo.IMAGENET_STD)
        self._fast_train = None                      # a captured step was captured without the matcher
        return self

    def _build_stereo_depth(self, batch, step_type):
        return self.gpu_stereo is not None and self.use_stereo_depth_gt and self.trans_2d_to_3d == "flosp_depth" \
            and step_type != "test" and self._tables_absent(batch, "gt_depth")

    def stereo_depth_on_gpu(self, batch):
        """The left camera's depth map of the batch's stereo pair -> (B, 1, H, W) float32 metres, 0 = no measurement
        (`enable_stereo_depth` describes the matcher and its assumptions).  Device calibration, no host read."""
        from .. import stereo
        if self.gpu_stereo is None:
            raise RuntimeError("stereo_depth_on_gpu: call enable_stereo_depth() first (or set OCCDEPTH_GPU_STEREO=1)")
        if self.dataset != "kitti":
            raise NotImplementedError("the stereo depth target is matched on the GPU for SemanticKITTI's rectified pair "
                                      "only; a %s batch must bring `gt_depth`" % self.dataset)
        missing = [k for k in ("cam_k", "T_velo_2_cam") if k not in batch]
        if missing:
            raise KeyError("stereo depth on the GPU needs the pair's calibration in the batch; missing: %s"
                           % ", ".join(missing))
        pair = batch["img_gray_u8"] if "img_gray_u8" in batch else batch["img"]
        if pair.dim() < 4 or pair.shape[1] != 2:
            raise ValueError("stereo depth on the GPU needs both views of the pair: `%s` has %s view(s) (shape %s)"
                             % ("img_gray_u8" if "img_gray_u8" in batch else "img",
                                pair.shape[1] if pair.dim() > 1 else 0, tuple(pair.shape)))
        if not pair.is_cuda:
            raise RuntimeError("the stereo depth target is matched on the GPU only (csrc/stereo.hip); a CPU batch must "
                               "bring `gt_depth`")
        dev = pair.device
        ext = batch.get("T_velo_2_cam_f64", batch["T_velo_2_cam"])
        E = torch.stack([e.to(dev) for e in ext]).to(torch.float64).contiguous()
        k = torch.stack([c.to(dev) for c in batch["cam_k"]]).to(torch.float64).contiguous()
        if E.dim() != 4 or E.shape[1] < 2 or k.shape[:2] != E.shape[:2]:
            raise ValueError("stereo depth on the GPU needs the calibration of both cameras: cam_k %s, T_velo_2_cam %s"
                             % (tuple(k.shape), tuple(E.shape)))
        ida = batch.get("ida_mats")
        if ida is not None:
            ida = (torch.stack([t.to(dev) for t in ida]) if isinstance(ida, (list, tuple)) else ida.to(dev)).to(torch.float32)
        return stereo.stereo_depth(pair, k, E, ida=ida, **self.gpu_stereo)

    # ---------------------------------------------------------------- depth-rendering loss (K36)
    def enable_render_loss(self, weight=1.0, stride=4, max_depth=None, norm="abs"):
        """Add `weight` x the depth-rendering loss (loss/render_loss.py: csrc/render_loss.hip on the GPU) to the train and val
        loss of every step that has a `gt_depth` -- the batch's, or the one `enable_stereo_depth` matches: `ssc_logit`'s
        soft occupancy is alpha-composited along every `stride`-th pixel ray of the left camera into an expected depth
        image and held to `gt_depth` (|d^ - D|, or that over D with norm="rel"), over the rays that have a measurement
        within `max_depth` metres (default: the upper depth bound of the dataset's FLoSP-Depth configuration; at most 128).
        Logged: <step_type>/loss_render (weighted, like the other terms); in val also <step_type>/render_abs_rel and
        <step_type>/render_rmse of the rendered depth over the valid rays.  Frames the loader mirrored
        (ida_mats[b, 0, 0, 0] < 0) are rendered through the mirrored view, chosen on the device: no host read, so the
        captured fast training step includes the loss.  SemanticKITTI geometry only.  A step without `gt_depth` logs and
        adds nothing.  The same switch from the environment: OCCDEPTH_RENDER_LOSS=<weight>[,<stride>]."""
        if self.dataset != "kitti":
            raise NotImplementedError("the depth-rendering loss is wired for the SemanticKITTI camera geometry only, not "
                                      "for a %s model" % self.dataset)
        from ..loss.render_loss import RenderDepthLoss
        if max_depth is None:
            max_depth = float(flosp_depth_conf_map[self.dataset]["d_bound"][1])
        if not float(weight) > 0.0:
            raise ValueError("enable_render_loss: weight must be > 0, got %r" % (weight,))
        self.render_loss = {"weight": float(weight), "fn": RenderDepthLoss(stride=stride, max_depth=max_depth, norm=norm)}
        self._fast_train = None                      # a captured step was captured without the loss
        return self

    def _render_loss_views(self, batch, ssc_pred, width):
        """One camera view per frame at the logits' own voxel size, mirrored where the loader mirrored the frame."""
        from .. import render
        from ..loss.render_loss import frame_views
        dev = ssc_pred.device
        vs = self.RENDER_VOXEL_METRES["kitti"] * float(self.full_scene_size[0]) / float(ssc_pred.shape[2])
        # the origin as a device tensor, made once per (origin, device) -- in the warm-up steps of a captured step, never inside
        # the capture: a host tuple would be copied to the device by every call, which a capture forbids
        origin = self._kitti_origin(batch)
        cache = self.render_loss.setdefault("origin", {})
        if (origin, str(dev)) not in cache:
            cache[(origin, str(dev))] = torch.tensor(origin, dtype=torch.float64, device=dev)
        k, E, origin = render.batch_camera(batch, self.dataset, cache[(origin, str(dev))], dev)
        ida = batch.get("ida_mats")
        flip = None
        if ida is not None:
            ida = torch.stack([t.to(dev) for t in ida]) if isinstance(ida, (list, tuple)) else ida.to(dev)
            flip = ida.reshape(ida.shape[0], -1, 4, 4)[:, 0, 0, 0] < 0
        return frame_views(k, E, origin, vs, width=width, flip=flip)

    def _render_loss_step(self, step_type, batch, ssc_pred, gt_depth):
        """-> the weighted loss term (logged), or None when this step has no depth target."""
        if gt_depth is None or gt_depth.numel() == 0 or step_type not in ("train", "val"):
            return None
        st = self.render_loss
        gt_depth = gt_depth.to(ssc_pred.device).float()
        gt_depth = gt_depth.reshape(gt_depth.shape[0], -1, *gt_depth.shape[-2:])[:, :1]          # the left camera's map
        views = self._render_loss_views(batch, ssc_pred, int(gt_depth.shape[-1]))
        fn = st["fn"]
        loss = fn(ssc_pred, gt_depth, views) * st["weight"]
        self._log(step_type + "/loss_render", loss)
        if step_type == "val":
            depth = fn.last[0]
            valid, target = fn.valid_rays(gt_depth, views, ssc_pred.shape[2:])
            n = valid.sum().clamp(min=1).float()
            err = (depth - target) * valid
            self._log(step_type + "/render_abs_rel", (err.abs() / target.clamp(min=1e-3)).sum() / n)
            self._log(step_type + "/render_rmse", ((err * err).sum() / n).sqrt())
        return loss

    # ---------------------------------------------------------------- Lovasz-softmax loss (K38)
    def enable_lovasz_loss(self, weight=1.0, class_chunk=None):
        """Add `weight` x the Lovasz-softmax loss of `ssc_logit` against the step's target (loss/lovasz_loss.py: csrc/sort.hip
        and csrc/lovasz.hip on the GPU) to the train and val loss: the convex surrogate of the per-class Jaccard index, over
        the whole batch and the classes present, label 255 unknown.  Logged: <step_type>/loss_lovasz (weighted, like the
        other terms).  It needs logits and target only: every dataset.  No host read, so the captured fast training step
        includes it.  class_chunk: classes sorted at a time over one scratch (default: all; `hip.lovasz_scratch_bytes`).
        The same switch from the environment: OCCDEPTH_LOVASZ=<weight>."""
        if not float(weight) > 0.0:
            raise ValueError("enable_lovasz_loss: weight must be > 0, got %r" % (weight,))
        from ..loss.lovasz_loss import LovaszSoftmaxLoss
        self.lovasz_loss = {"weight": float(weight), "fn": LovaszSoftmaxLoss(class_chunk=class_chunk)}
        self._fast_train = None                      # a captured step was captured without the loss
        return self

    # ---------------------------------------------------------------- whole-forward hipGraph
    @staticmethod
    def _batch_signature(batch):
        sig = []
        for k in sorted(batch):
            v = batch[k]
            if torch.is_tensor(v):
                sig.append((k, tuple(v.shape), v.dtype, v.device))
            elif isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) for t in v):
                sig.append((k, tuple((tuple(t.shape), t.dtype, t.device) for t in v)))
        return tuple(sig)

    @staticmethod
    def _copy_batch(dst, src):
        for k, v in src.items():
            d = dst.get(k)
            if torch.is_tensor(v) and torch.is_tensor(d):
                if d.data_ptr() != v.data_ptr():
                    d.copy_(v, non_blocking=True)
            elif isinstance(v, (list, tuple)) and isinstance(d, list):
                for dd, vv in zip(d, v):
                    if torch.is_tensor(vv) and dd.data_ptr() != vv.data_ptr():
                        dd.copy_(vv, non_blocking=True)

    def _forward_graphed(self, batch):
        """`graph_all` (opt-in, eval under no_grad, GPU batch): the WHOLE forward -- 2-D network, FLoSP-Depth, lift, 3-D
        stack -- captured once per batch signature into ONE hipGraph and replayed per frame: the host only copies the
        frame's tensors into the graph's static inputs (~20 MB at config 2) and launches the replay, so no launch gap is
        left between the 2-D network, the lift and the 3-D stack (rocprof r02: 1.4 ms of a 26.8 ms frame).  The returned
        tensors are the graph's static outputs: valid until the next forward of this model (clone what must survive).
        Like `graph_2d`, an entry is re-captured when any parameter / buffer changed (exact (_version, data_ptr) stamp),
        and a failed capture falls back to the eager path with a warning (`graph_all_error`)."""
        key = ("all", self._batch_signature(batch))
        stamp = self._stamp_of(self, "_all_tensors")
        entry = self._graphs.get(key)
        if entry is not None and entry[3] != stamp:
            entry = None
        if entry is None:
            static = {k: (v.clone() if torch.is_tensor(v) else
                          [t.clone() if torch.is_tensor(t) else t for t in v] if isinstance(v, (list, tuple)) else v)
                      for k, v in batch.items()}
            dev = batch["img"].device
            try:
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    for _ in range(2):                         # warm-up: plans, packed weights, library solvers, K2s counters
                        self._forward_impl(static, allow_graph_2d=False)
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize(dev)
                graph = new_graph()
                with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
                    static_out = self._forward_impl(static, allow_graph_2d=False)
                seal_graph(graph)
                entry = (graph, static, static_out, stamp)
            except (RuntimeError, torch.AcceleratorError) as e:   # capture is an optimisation, never a requirement
                import warnings
                warnings.warn(f"occdepth_amd: hipGraph capture of the whole forward failed ({e!r}); running eagerly")
                self.graph_all = False
                self.graph_all_error = repr(e)
                torch.cuda.synchronize(dev)
                return self._forward_impl(batch)
            self._graphs[key] = entry
        graph, static, static_out, _ = entry
        self._copy_batch(static, batch)
        graph.replay()
        if self.clone_graph_outputs:
            return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in static_out.items()}
        return dict(static_out)

    def forward(self, batch):
        if self.graph_all and not needs_autograd(self) and batch["img"].is_cuda \
                and not torch.cuda.is_current_stream_capturing():
            return self._forward_graphed(batch)
        return self._forward_impl(batch)

    def _forward_impl(self, batch, allow_graph_2d=True):
        if allow_graph_2d or not self.graph_2d:
            return self._forward_body(batch)
        self.graph_2d = False                  # (the whole-forward capture contains the 2-D network: no nested replay)
        try:
            return self._forward_body(batch)
        finally:
            self.graph_2d = True

    def _forward_body(self, batch):
        img = batch["img"].to(device)
        bs, n_views = img.shape[:2]
        x_rgb, n_views = self.process_rgbs(img, batch, n_views)
        if self.dataset in ("NYU", "tartanair"):
            vox_origin = batch["vox_origin"]
        elif self.dataset == "kitti":
            vox_origin = None
        else:
            raise NotImplementedError("dataset is not supported: {}".format(self.dataset))
        x3ds, depth_pred = self._forward_2d_to_3d(batch, x_rgb, img, bs, vox_origin)
        out = dict(self.net_3d_decoder({"x3d": x3ds}))
        if self.with_depth_gt and self.trans_2d_to_3d == "flosp_depth":
            out["depth_pred"] = depth_pred
        return out

    # ---------------------------------------------------------------- Lightning hooks
    def _log(self, key, value):
        self.logged[key] = value.detach()
        # inside the fast training step (its capture, its warm-up steps on a snapshot, its eager fall-back) the Trainer's
        # logger is fed AFTER the step from `self.logged` (_fast_training_step): a logger call inside a capture would be
        # baked into the graph -- or synchronise the host, which a capture forbids
        if not self.__dict__.get("_in_fast_step", False):
            self.log(key, value.detach(), on_epoch=True, sync_dist=True)

    def step(self, batch, step_type, metric):
        """Loss assembly of occdepth/models/OccDepth.py:378-533.  Same terms, same switches, same log keys; the
        scene-completion terms (CE, sem_scal, geo_scal, frustum proportion) come from one statistics pass over
        `ssc_logit` (loss/ssc_loss.py), and the metric update stays on the GPU (no `.cpu().numpy()` per step)."""
        from ..loss import ssc_loss
        from ..loss.CRP_loss import compute_super_CP_multilabel_loss
        self.logged = {}
        out_dict = self(batch)
        ssc_pred = out_dict["ssc_logit"]
        dev = ssc_pred.device
        target, occluded = self._step_labels(batch, dev)
        use_rel = self.context_prior and self.relation_loss
        built_fp = built_cp = None
        if self.fp_loss and step_type != "test" and self._build_target(batch, "frustums_masks"):
            built_fp = self.frustum_targets_on_gpu(batch, target)
        if use_rel and self._build_target(batch, "CP_mega_matrices"):
            built_cp = self.relation_targets_on_gpu(target)
        loss = 0
        if use_rel:
            loss_rel_ce = compute_super_CP_multilabel_loss(out_dict["P_logits"],
                                                           built_cp if built_cp is not None else batch["CP_mega_matrices"])
            loss = loss + loss_rel_ce
            self._log(step_type + "/loss_relation_ce_super", loss_rel_ce)

        use_fp = self.fp_loss and step_type != "test"
        masks = dists = None
        if use_fp:
            if built_fp is not None:
                masks, dists = built_fp
            else:
                masks = torch.stack(list(batch["frustums_masks"])).to(dev)
                dists = torch.stack(list(batch["frustums_class_dists"])).float().to(dev)
        terms = ssc_loss.ssc_losses(ssc_pred, target, self._on_device("class_weights", dev), masks, dists,
                                    ce=self.CE_ssc_loss, sem_scal=self.sem_scal_loss, geo_scal=self.geo_scal_loss)
        if self.CE_ssc_loss:
            loss = loss + terms["loss_ssc"]
            self._log(step_type + "/loss_ssc", terms["loss_ssc"])
            if self.cascade_cls:
                loss_occ = ssc_loss.occ_ce_loss(out_dict["occ_logit"], target, self._on_device("class_weights_occ", dev))
                loss = loss + loss_occ
                self._log(step_type + "/loss_occ", loss_occ)
            if self.occluded_cls and occluded is not None:
                loss_occluded = ssc_loss.CE_ssc_loss(out_dict["occluded_logit"], occluded,
                                                     torch.ones(2, device=dev))
                loss = loss + loss_occluded
                self._log(step_type + "/loss_occluded", loss_occluded)

        gt_depth = batch["gt_depth"] if "gt_depth" in batch else None
        if self.gpu_stereo is not None and self._tables_absent(batch, "gt_depth"):
            # matched from the batch's image pair (the batch is not changed); a hooked loader's zero-size map is no target
            gt_depth = self.stereo_depth_on_gpu(batch) if self._build_stereo_depth(batch, step_type) else None
        if self.with_depth_gt and self.trans_2d_to_3d == "flosp_depth" and gt_depth is not None:
            if self.use_stereo_depth_gt:
                depth_pred = out_dict["depth_pred"][:, 0].unsqueeze(1)        # only the left camera has ground truth
            elif self.use_lidar_depth_gt or self.use_depth_gt:
                depth_pred = out_dict["depth_pred"]
            else:
                raise NotImplementedError("Only stereo depth gt supported.")
            loss_depth = self.depth_loss_fn.get_depth_loss(gt_depth.to(dev), depth_pred) * self.depth_loss_w
            loss = loss + loss_depth
            self._log(step_type + "/loss_depth", loss_depth)

        if self.render_loss is not None:
            loss_render = self._render_loss_step(step_type, batch, ssc_pred, gt_depth)
            if loss_render is not None:
                loss = loss + loss_render

        if getattr(self, "lovasz_loss", None) is not None and step_type in ("train", "val"):
            loss_lovasz = self.lovasz_loss["fn"](ssc_pred, target) * self.lovasz_loss["weight"]
            loss = loss + loss_lovasz
            self._log(step_type + "/loss_lovasz", loss_lovasz)

        if self.sem_scal_loss:
            decay = max(0.1, (1 - self.cur_batch / self.total_batch)) if self.sem_step_decay_loss else 1.0
            if self.sem_step_decay_loss and getattr(self, "_decay_dev", None) is not None and ssc_pred.is_cuda:
                # device scalar a captured step reads (train_graph.GraphedTrainStep refreshes it before every replay).  An
                # EAGER step -- a failed capture's fall-back, or a plain training_step once the scalar exists -- refreshes it
                # here from the host formula (asynchronous fill, no sync), so the factor can never freeze at its capture value
                if not torch.cuda.is_current_stream_capturing():
                    self._decay_dev.fill_(decay)
                decay = self._decay_dev
            loss_sem_scal = terms["loss_sem_scal"] * decay
            loss = loss + loss_sem_scal
            self._log(step_type + "/loss_sem_scal", loss_sem_scal)
        if self.geo_scal_loss:
            loss = loss + terms["loss_geo_scal"]
            self._log(step_type + "/loss_geo_scal", terms["loss_geo_scal"])
        if use_fp:
            loss = loss + terms["loss_frustums"]
            self._log(step_type + "/loss_frustums", terms["loss_frustums"])

        if metric is not None:
            if hasattr(metric, "add_batch_logits"):
                metric.add_batch_logits(ssc_pred, target)
            else:                                        # a reference-style (numpy) metric object
                metric.add_batch(ssc_pred.detach().argmax(1).cpu().numpy(), target.cpu().numpy())
        if self.eval_report is not None and step_type in ("test", "val"):
            self._report_count(step_type, batch, ssc_pred, target)
        fused_labels = None
        if self.temporal_fusion is not None and step_type in ("test", "val"):
            fused_labels = self._fuse_step(step_type, batch, ssc_pred, target)
        ray_on = getattr(self, "ray_metrics", None) is not None and step_type in ("test", "val")
        dist_on = getattr(self, "dist_metrics", None) is not None and step_type in ("test", "val")
        if ray_on and dist_on:                                        # one arg-max of the unfused logits for both
            from .. import hip
            pred_labels = hip.argmax_labels_u16(ssc_pred.detach().float())
            self._ray_step(step_type, batch, ssc_pred, target, fused_labels, pred_labels=pred_labels)
            self._dist_step(step_type, batch, ssc_pred, target, fused_labels, pred_labels=pred_labels)
        elif ray_on:
            self._ray_step(step_type, batch, ssc_pred, target, fused_labels)
        elif dist_on:
            self._dist_step(step_type, batch, ssc_pred, target, fused_labels)
        if getattr(self, "panoptic_metrics", None) is not None and step_type in ("test", "val"):
            self._pan_step(step_type, batch, ssc_pred, target, fused_labels)
        if getattr(self, "semantic_map", None) is not None and step_type in ("test", "val"):
            self._map_step(step_type, batch, ssc_pred, target)
        self._log(step_type + "/loss", loss)
        if self.render is not None and step_type in ("test", "val"):
            self._render_step(step_type, batch, ssc_pred, target)     # last: its copy waits for the step's kernels
        return loss

    @staticmethod
    def _targets():
        from .. import targets
        return targets

    def _build_target(self, batch, key):
        """OCCDEPTH_GPU_TARGETS: is target `key` built on the GPU for this batch?"""
        if self.gpu_targets is True:
            return True
        if self.gpu_targets is False:
            return False
        return self._tables_absent(batch, key)

    def _step_labels(self, batch, dev):
        """(target, occluded or None) of a step, on `dev`.  A batch that brings `target` is used as it is (with its
        `occluded`, when it has one).  Without `target` (missing, empty list or zero elements: _tables_absent) the batch must
        bring the dataset's raw voxel files -- `voxel_label_raw` (B, N) uint16 or int16, `voxel_invalid_bits` (B, N / 8)
        uint8 and, for `occluded_cls`, `voxel_occluded_bits` -- which targets.kitti_labels decodes on the GPU, eagerly or
        inside a captured step; the frustum and relation targets are then built from the decoded labels as for any batch
        without them.  The batch itself is not changed (a captured step keeps its static keys)."""
        if not self._tables_absent(batch, "target"):
            occluded = batch.get("occluded") if self.occluded_cls else None
            return batch["target"].to(dev), (occluded.to(dev) if occluded is not None else None)
        if "voxel_label_raw" not in batch or "voxel_invalid_bits" not in batch:
            raise KeyError("the batch brings neither `target` nor the raw voxel files (`voxel_label_raw`, "
                           "`voxel_invalid_bits`) to decode it from")
        if self.gpu_targets is False:
            raise RuntimeError("the batch brings raw voxel files instead of `target`; decoding them is part of building the "
                               "training targets on the GPU (OCCDEPTH_GPU_TARGETS=auto or 1), not OCCDEPTH_GPU_TARGETS=0")
        if self.dataset != "kitti":
            raise NotImplementedError("raw voxel labels are decoded on the GPU for SemanticKITTI only; a %s batch must "
                                      "bring `target`" % self.dataset)
        scale = -(-int(self.project_scale) // 2)
        dims = tuple(int(d) // scale for d in self.full_scene_size)

        def rows(key):
            v = batch[key]
            return [t.to(dev) for t in v] if isinstance(v, (list, tuple)) else v.to(dev)

        occ_bits = rows("voxel_occluded_bits") if self.occluded_cls and "voxel_occluded_bits" in batch else None
        out = self._targets().kitti_labels(rows("voxel_label_raw"), rows("voxel_invalid_bits"), occ_bits, scene_size=dims)
        return out if occ_bits is not None else (out, None)

    def frustum_targets_on_gpu(self, batch, target):
        """(frustums_masks (B, F, X, Y, Z) bool, frustums_class_dists (B, F, C) float32) of kitti_dataset.py:315-333, built
        on the GPU (targets.frustum_targets) from the batch's UNFLIPPED calibration -- the reference builds them before its
        flip augmentation (:384), so the batch's (possibly flipped) projected_pix tables are never used.  Output scale
        ceil(project_scale / 2) (kitti_dataset.py:83), SemanticKITTI origin (_kitti_origin)."""
        if self.dataset != "kitti":
            raise NotImplementedError("frustum targets are built on the GPU for the SemanticKITTI geometry only; a %s batch "
                                      "must bring frustums_masks / frustums_class_dists" % self.dataset)
        scale = -(-int(self.project_scale) // 2)
        dims = tuple(int(d) // scale for d in self.full_scene_size)
        if target.dim() != 4 or tuple(target.shape[1:]) != dims:
            raise NotImplementedError("frustum targets on the GPU: target grid %s does not match the output grid %s; the "
                                      "batch must bring frustums_masks / frustums_class_dists" % (tuple(target.shape[1:]), dims))
        dev = target.device
        ext = batch.get("T_velo_2_cam_f64", batch.get("T_velo_2_cam"))
        E = torch.stack([e.to(dev) for e in ext]).to(torch.float64)
        k = torch.stack([c.to(dev) for c in batch["cam_k"]]).to(torch.float64)
        H, W = batch["img"].shape[-2:]
        return self._targets().frustum_targets(E, k, target, vox_origin=self._kitti_origin(batch), voxel_size=0.2 * scale,
                                               img_wh=(int(W), int(H)), frustum_size=self.frustum_size,
                                               n_classes=self.n_classes)

    def relation_targets_on_gpu(self, target):
        """CP_mega_matrices (B, 4, N, M) uint8 of kitti_dataset.py:294-300, built on the GPU: the 4-way matrix
        (targets.cp_mega_matrix) of the 1:8 labels, which the reference's preprocessing makes from the 1:1 labels with
        _downsample_label (targets.downsample_label)."""
        if self.dataset != "kitti":
            raise NotImplementedError("relation targets are built on the GPU for the SemanticKITTI geometry only (NYU's come "
                                      "from a 1:16 label the batch does not carry); the batch must bring CP_mega_matrices")
        if target.dim() != 4 or any(int(d) % 16 for d in target.shape[1:]):
            raise NotImplementedError("relation targets on the GPU need a (B, X, Y, Z) target with X, Y, Z multiples of 16, "
                                      "got %s; the batch must bring CP_mega_matrices" % (tuple(target.shape),))
        t = self._targets()
        return t.cp_mega_matrix(t.downsample_label(target, 8))

    def _on_device(self, name, dev):
        """float32 device copy of a host-side attribute tensor (class weights), cached: `.to(dev)` per step is a host
        sync on the loss path."""
        src = getattr(self, name)
        cache = self.__dict__.setdefault("_dev_attr", {})
        hit = cache.get((name, str(dev)))
        if hit is None or hit[0] is not src:
            hit = (src, src.to(dev).float())
            cache[(name, str(dev))] = hit
        return hit[1]

    def training_step(self, batch, batch_idx):
        if self.fast_train and not self.__dict__.get("_in_fast_step", False):
            return self._fast_training_step(batch, batch_idx)
        self.cur_batch += 1
        return self.step(batch, "train", self.train_metrics)

    # ---- OCCDEPTH_FAST_TRAIN: the benched training step behind the Trainer's `training_step`
    @staticmethod
    def _batch_signature(batch):
        sig = []
        for k in sorted(batch):
            v = batch[k]
            if torch.is_tensor(v):
                sig.append((k, tuple(v.shape), v.dtype))
            elif isinstance(v, (list, tuple)) and v and all(torch.is_tensor(t) for t in v):
                sig.append((k, tuple((tuple(t.shape), t.dtype) for t in v)))
            else:
                sig.append((k, repr(v) if isinstance(v, (int, float, str, bool, type(None))) else type(v).__name__))
        return tuple(sig)

    def _fast_optimizer(self):
        """The raw torch optimizer of this module: the one `configure_optimizers` built (Lightning calls it before the first
        step), else what the Trainer reports through `self.optimizers()`."""
        if self._opt is not None:
            return self._opt
        opts = self.optimizers()
        opt = opts[0] if isinstance(opts, (list, tuple)) else opts
        return getattr(opt, "optimizer", opt)

    def _grad_clip_value(self):
        """The global gradient-norm clip of the fast training step, first hit wins: `enable_fast_train(grad_clip=...)`, then
        the attached Trainer's `gradient_clip_val` (every reference yaml: 35, scripts/train.py:188,204) -- with
        `automatic_optimization = False` Lightning 1.4.9 skips its own clipping together with backward and optimizer.step.
        None or 0: no clipping.  Clipping by value is not implemented and raises instead of being ignored."""
        from .. import optim
        if self.fast_train_grad_clip is not None:
            return self.fast_train_grad_clip if optim.clipping_enabled(self.fast_train_grad_clip) else None
        try:
            trainer = getattr(self, "trainer", None)
        except RuntimeError:                                 # newer Lightning: the property raises while no Trainer is attached
            trainer = None
        val = getattr(trainer, "gradient_clip_val", None)
        if trainer is None or not optim.clipping_enabled(val):
            return None
        algo = getattr(trainer, "gradient_clip_algorithm", None)
        if str(getattr(algo, "value", algo)).lower() == "value":
            raise NotImplementedError("occdepth_amd: the fast training step clips gradients by global norm only "
                                      "(Trainer(gradient_clip_algorithm='value') is not implemented)")
        return float(val)

    @staticmethod
    def _check_accumulate(n, where):
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"occdepth_amd: {where} must be an int >= 1, got {n!r}")
        return n

    def _accumulate_value(self):
        """N of the fast training step's gradient accumulation, first hit wins: `enable_fast_train(accumulate=...)`, then
        OCCDEPTH_FAST_TRAIN_ACCUM in the environment (the route for an unmodified scripts/train.py, whose Trainer(...) call
        passes no `accumulate_grad_batches`), then the attached Trainer's `accumulate_grad_batches`, else 1.  With
        `automatic_optimization = False` Lightning 1.4.9 skips accumulation together with backward, clipping and
        optimizer.step.  Anything but an int >= 1 (a per-epoch schedule dict among them) raises ValueError."""
        if self.fast_train_accumulate is not None:
            return self._check_accumulate(self.fast_train_accumulate, "enable_fast_train(accumulate=...)")
        env = os.environ.get("OCCDEPTH_FAST_TRAIN_ACCUM")
        if env is not None and env.strip() != "":
            try:
                n = int(env.strip())
            except ValueError:
                raise ValueError(f"occdepth_amd: OCCDEPTH_FAST_TRAIN_ACCUM must be an int >= 1, got {env!r}") from None
            return self._check_accumulate(n, "OCCDEPTH_FAST_TRAIN_ACCUM")
        try:
            trainer = getattr(self, "trainer", None)
        except RuntimeError:                                 # newer Lightning: the property raises while no Trainer is attached
            trainer = None
        if trainer is None:
            return 1
        return self._check_accumulate(getattr(trainer, "accumulate_grad_batches", 1), "Trainer(accumulate_grad_batches=...)")

    def _window_position(self, st, batch_idx):
        """pytorch-lightning 1.4.9's rule under automatic optimisation (TrainingBatchLoop.should_accumulate): the window
        closes when (batch_idx + 1) % N == 0 or with the epoch's last batch; the scale stays 1/N for an epoch's short last
        window.  It opens at batch_idx % N == 0 -- or wherever no window is open on the host (a run resumed in the middle
        of a window must not read accumulators nobody wrote)."""
        n = self._accumulate_value()
        if n != st["accumulate"]:
            raise ValueError(f"occdepth_amd: gradient accumulation changed from {st['accumulate']} to {n} after the first fast "
                             "training step; call enable_fast_train() again to start over")
        w = st["window"]
        if w is None:
            return
        try:
            trainer = getattr(self, "trainer", None)
        except RuntimeError:
            trainer = None
        last = (batch_idx + 1) % n == 0 or batch_idx + 1 == getattr(trainer, "num_training_batches", None)
        w.set(batch_idx % n == 0 or not w.is_open, last)

    def _fast_training_step(self, batch, batch_idx):
        """`training_step` under manual optimisation (`automatic_optimization = False`: Lightning 1.4.9 then calls neither
        backward nor optimizer.step, models/OccDepth.py:535-541 + scripts/train.py:208 otherwise drive them eagerly).
        First call: the batch becomes the STATIC batch of a `GraphedTrainStep` (device copies), the step is captured (its
        warm-up steps run on a snapshot: capturing trains nothing) and replayed; later calls copy the new batch into the
        static tensors and replay.  Several ranks: the module is wrapped in DDP by the Trainer, whose reducer only acts on a
        backward that follows the forward -- here the backward is INSIDE the step, so the gradient average is taken by
        `shard.GradBuckets` (captured with the step) and DDP's hooks stay idle.  What the replay cannot do is done here:
        `self.log` of the step's loss terms (device scalars the graph writes), the host counters (GraphedTrainStep.__call__).
        Falls back to the eager manual step with a warning when the capture fails, on the CPU, or for a batch whose
        keys / shapes differ from the captured one (that batch alone runs eagerly).
        Gradient accumulation (`_accumulate_value` = N > 1): every call is one micro-batch of a window of N
        (`_window_position`); replayed and eager micro-batches share ONE `optim.GradWindow` of the optimizer, so a window
        may mix them.  With `GradBuckets` the all-reduce runs every micro-batch -- correct, averaging is linear; skipping it
        on the micro-batches that do not close a window is not done."""
        import warnings
        from .. import autograd3d, optim, shard, train_graph
        on_gpu = next(self.parameters()).is_cuda
        opt = self._fast_optimizer()
        st = self._fast_train
        if st is None:
            n_acc = self._accumulate_value()
            st = self._fast_train = {"graph": None, "sig": None, "buckets": None, "warned": False, "logged": None,
                                     "accumulate": n_acc, "window": optim.GradWindow(opt, n_acc) if n_acc > 1 else None}
            if on_gpu:
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                    st["buckets"] = shard.GradBuckets(self.parameters(), dist)
                dev = next(self.parameters()).device
                static = {k: ([t.to(dev).clone() if torch.is_tensor(t) else t for t in v] if isinstance(v, (list, tuple))
                              else (v.to(dev).clone() if torch.is_tensor(v) else v)) for k, v in batch.items()}
                if self.fast_train_bf16:
                    autograd3d.set_bf16_mfma(True)
                gs = train_graph.GraphedTrainStep(self, opt, static, bf16=self.fast_train_autocast, buckets=st["buckets"],
                                                  warmup=2, batch_idx=batch_idx, grad_clip=self._grad_clip_value(),
                                                  accumulate=n_acc, window=st["window"])
                self.__dict__["_in_fast_step"] = True
                try:
                    ok = gs.capture()
                finally:
                    self.__dict__["_in_fast_step"] = False
                st["graph"], st["sig"] = gs, self._batch_signature(static)
                st["logged"] = dict(self.logged) if ok else None     # the device scalars the captured step writes
                if not ok:
                    warnings.warn(f"occdepth_amd: the training step could not be captured ({gs.error}); running it eagerly")
            else:
                warnings.warn("occdepth_amd: OCCDEPTH_FAST_TRAIN needs the model on the GPU; running the eager manual step")
        gs = st["graph"]
        self._window_position(st, batch_idx)
        self.__dict__["_in_fast_step"] = True
        try:
            if gs is not None and self._batch_signature(batch) == st["sig"]:
                gs.load_batch(batch)
                loss = gs()                                  # replay (or the eager step on the static batch after a failed capture)
                if gs.graph is not None:
                    self.logged = dict(st["logged"])
            else:
                if gs is not None and not st["warned"]:
                    st["warned"] = True
                    warnings.warn("occdepth_amd: a training batch differs in keys / shapes from the captured one; such "
                                  "batches run the eager step")
                loss = self._manual_eager_step(batch, batch_idx, opt, st["buckets"])
        finally:
            self.__dict__["_in_fast_step"] = False
        for k, v in self.logged.items():                    # the replay does not run Python: log what the graph wrote
            self.log(k, v, on_epoch=True, sync_dist=True)
        return loss.detach()

    def _manual_eager_step(self, batch, batch_idx, opt, buckets=None):
        """One manual-optimisation step without a graph: zero_grad, training_step, backward, [gradient average], optimizer
        -- with a clip value set (`_grad_clip_value`), `optim.clip_adamw_step`: clip_grad_norm_ + AdamW, norm logged.
        With gradient accumulation the optimizer stage is one micro-batch of the step's window (`_fast_training_step`)."""
        if buckets is not None:
            buckets.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bool(self.fast_train_autocast and next(self.parameters()).is_cuda)):
            loss = self.training_step(batch, batch_idx)
        loss.backward()
        if buckets is not None:
            buckets.finish()
        clip = self._grad_clip_value()
        window = (self._fast_train or {}).get("window")
        if window is not None:
            from .. import optim
            norm = optim.clip_adamw_step(opt, clip, window=window)
            if norm is not None:                             # the last closed window's
                self._log("train/grad_norm", norm)
        elif clip is None:
            opt.step()
        else:
            from .. import optim
            self._log("train/grad_norm", optim.clip_adamw_step(opt, clip))
        return loss

    def on_train_epoch_start(self, *args, **kwargs):
        """Manual optimisation: Lightning 1.4 leaves the LR schedule to the module.  MultiStepLR counts epochs: bring it to
        the current epoch (idempotent -- a Trainer that did step it finds nothing to do)."""
        if not self.fast_train or self._sched is None:
            return
        epoch = int(getattr(self, "current_epoch", 0) or 0)
        while self._sched.last_epoch < epoch:
            self._sched.step()

    def on_train_batch_end(self, *args, **kwargs):
        """Once per step (Lightning calls it after backward + optimizer step): a peer-memory SyncBatchNorm exchange that
        gave up waiting for a rank raises here instead of training on -- its results are already NaN (shard.SmallAllReduce).
        No host synchronisation: the device flag is copied asynchronously and examined one step later."""
        from .. import shard
        shard.poll_exchanges()

    def validation_step(self, batch, batch_idx):
        self.step(batch, "val", self.val_metrics)

    def _epoch_stats(self, metric):
        """`SSCMetrics.get_stats()` of this rank's counts -- the reference's semantics: each rank logs the statistics of
        its own confusion matrix and Lightning averages them (`sync_dist=True`).  With `metrics_allreduce` the
        confusion matrices are summed over the ranks first (the statistically exact variant)."""
        if self.metrics_allreduce:
            from .. import shard
            shard.allreduce_confusion(metric)
        return metric.get_stats()

    def validation_epoch_end(self, outputs):
        """Reference :542-557: per-class IoU, mIoU, IoU, Precision, Recall of the train and val metrics, then reset."""
        for prefix, metric in (("train", self.train_metrics), ("val", self.val_metrics)):
            stats = self._epoch_stats(metric)
            for i, class_name in enumerate(self.class_names):
                self.log("{}_SemIoU/{}".format(prefix, class_name), stats["iou_ssc"][i], sync_dist=True)
            self.log("{}/mIoU".format(prefix), stats["iou_ssc_mean"], sync_dist=True)
            self.log("{}/IoU".format(prefix), stats["iou"], sync_dist=True)
            self.log("{}/Precision".format(prefix), stats["precision"], sync_dist=True)
            self.log("{}/Recall".format(prefix), stats["recall"], sync_dist=True)
            metric.reset()
        rep = self.report_metrics.get("val")
        if rep is not None:
            if self.metrics_allreduce and rep.region_hist is not None:
                from .. import shard
                shard.allreduce_confusion(rep.region_hist)
            for name, stats in rep.get_region_stats().items():
                self.log("val_region/{}/mIoU".format(name), stats["iou_ssc_mean"], sync_dist=True)
                self.log("val_region/{}/IoU".format(name), stats["iou"], sync_dist=True)
            rep.reset()
        fused = self.fused_metrics.get("val")
        if fused is not None:
            stats = self._epoch_stats(fused)
            self.log("val_fused/mIoU", stats["iou_ssc_mean"], sync_dist=True)
            self.log("val_fused/IoU", stats["iou"], sync_dist=True)
            fused.reset()
        if getattr(self, "semantic_map", None) is not None:
            stats = self._map_epoch_end("val")
            if stats is not None:
                self.log("val_map/mIoU", stats["iou_ssc_mean"], sync_dist=True)
                self.log("val_map/IoU", stats["iou"], sync_dist=True)
            stats = self.semantic_map.get("mapped_stats", {}).pop("val", None)
            if stats is not None:
                self.log("val_mapped/mIoU", stats["iou_ssc_mean"], sync_dist=True)
                self.log("val_mapped/IoU", stats["iou"], sync_dist=True)
        if getattr(self, "ray_metrics", None) is not None:
            for prefix, stats in self._ray_epoch_end("val"):
                self.log(prefix + "/RayIoU", stats["RayIoU"], sync_dist=True)
                for t, v in zip(stats["thresholds_m"], stats["ray_miou"]):
                    self.log("%s/RayIoU@%g" % (prefix, t), v, sync_dist=True)
                self.log(prefix + "/RayIoU_geo", stats["ray_iou_geo"].mean(), sync_dist=True)
        if getattr(self, "dist_metrics", None) is not None:
            for prefix, stats in self._dist_epoch_end("val"):
                for i, t in enumerate(stats["thresholds_m"]):
                    self.log("%s/F_geo@%g" % (prefix, t), stats["F_geo"][i], sync_dist=True)
                    self.log("%s/F_sem@%g" % (prefix, t), stats["F_sem"][i], sync_dist=True)
                self.log(prefix + "/CD_geo", stats["CD_geo"], sync_dist=True)
                self.log(prefix + "/CD_sem", stats["CD_sem"], sync_dist=True)
        if getattr(self, "panoptic_metrics", None) is not None:
            for prefix, stats in self._pan_epoch_end("val"):
                for key in ("PQ", "PQ_things", "PQ_stuff", "SQ", "RQ", "PQ_dagger"):
                    self.log("%s/%s" % (prefix, key), stats[key], sync_dist=True)
        if self.render is not None:
            self.render["logged"] = False           # the next epoch logs its first rendered frame again

    def test_step(self, batch, batch_idx):
        self.step(batch, "test", self.test_metrics)

    def test_epoch_end(self, outputs):
        """Reference :562-580: the printed evaluation report of scripts/eval.py."""
        classes = self.class_names
        fused = self.fused_metrics.get("test")
        for prefix, metric in (("test", self.test_metrics),) + ((("test_fused", fused),) if fused is not None else ()):
            print("{}======".format(prefix))
            stats = self._epoch_stats(metric)
            print("Precision={:.4f}, Recall={:.4f}, IoU={:.4f}".format(
                stats["precision"] * 100, stats["recall"] * 100, stats["iou"] * 100))
            print("class IoU: {}, ".format(classes))
            print(" ".join(["{:.4f}, "] * len(classes)).format(*(stats["iou_ssc"] * 100).tolist()))
            print("mIoU={:.4f}".format(stats["iou_ssc_mean"] * 100))
            metric.reset()
        self._print_region_report("test")
        if getattr(self, "semantic_map", None) is not None:
            stats = self._map_epoch_end("test")
            for prefix, stats in (("test_map", stats), ("test_mapped", self.semantic_map.get("mapped_stats", {}).pop("test", None))):
                if stats is not None:
                    print("{}======".format(prefix))
                    print("Precision={:.4f}, Recall={:.4f}, IoU={:.4f}".format(
                        stats["precision"] * 100, stats["recall"] * 100, stats["iou"] * 100))
                    print("class IoU: {}, ".format(classes))
                    print(" ".join(["{:.4f}, "] * len(classes)).format(*(stats["iou_ssc"] * 100).tolist()))
                    print("mIoU={:.4f}".format(stats["iou_ssc_mean"] * 100))
        if getattr(self, "ray_metrics", None) is not None:
            from ..ray_metric import format_report
            for prefix, stats in self._ray_epoch_end("test"):
                print("\n".join(format_report(stats, classes, prefix)))
        if getattr(self, "dist_metrics", None) is not None:
            from ..dist_metric import format_report as format_dist_report
            for prefix, stats in self._dist_epoch_end("test"):
                print("\n".join(format_dist_report(stats, classes, prefix)))
        if getattr(self, "panoptic_metrics", None) is not None:
            from ..panoptic import format_report as format_pan_report
            for prefix, stats in self._pan_epoch_end("test"):
                print("\n".join(format_pan_report(stats, classes, prefix)))

    def configure_optimizers(self):
        """Reference :582-600: AdamW + MultiStepLR, schedule by dataset."""
        from torch.optim.lr_scheduler import MultiStepLR
        if self.dataset in ("NYU", "kitti"):
            milestones, gamma = [18, 24], 0.4
        elif self.dataset == "tartanair":
            milestones, gamma = [20], 0.1
        else:
            raise NotImplementedError("dataset is not supported: {}".format(self.dataset))
        params = list(self.parameters())
        opt = None
        if params and all(p.is_cuda and p.is_floating_point() for p in params):
            try:        # the fused (multi-tensor, single-launch) implementation of the same AdamW update
                opt = torch.optim.AdamW(params, lr=self.lr, weight_decay=self.weight_decay, fused=True)
            except (RuntimeError, ValueError):
                opt = None
        if opt is None:
            opt = torch.optim.AdamW(params, lr=self.lr, weight_decay=self.weight_decay)
        self._opt = opt
        if self.fast_train and params and params[0].is_cuda:
            from .. import train_graph
            train_graph.make_capturable(opt)            # device-side step counter and learning rate, before the first step
        self._sched = MultiStepLR(opt, milestones=milestones, gamma=gamma)
        return [opt], [self._sched]
