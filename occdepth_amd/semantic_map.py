"""Sequence-level semantic map (K30): every frame's labelled voxels are laid into one sparse world-frame voxel map by
the ego-motion and voxels seen from several frames are decided by vote (csrc/semantic_map.hip: hip.map_integrate lets a
frame vote in one launch, hip.map_brick_labels / hip.map_extract decide).

    poses = fuse.read_kitti_poses(".../dataset/sequences/08")
    m = SemanticMap(20, 0.2, (0.0, -25.6, -2.0), (256, 256, 32))
    m.integrate(labels, poses[frame], mask=fov_mask_1)               # (X, Y, Z) uint8 / int16 on the GPU
    coords, labels, n_obs = m.extract(min_obs=2)
    write_ply("08.ply", coords, labels, n_obs, 0.2, render.palette("kitti"))
    map_confusion(pred_map, gt_map, SSCMetrics(20))                  # map mIoU where both maps were observed
    labels, n_obs = m.sample(poses[frame], own=labels, own_mask=fov_mask_1, keep_own=True)   # the map read back into a frame (K32)
    m.merge(other); m.save("08.occmap"); SemanticMap.load("08.occmap"); merge_over_ranks(m)   # maps summed: runs, files, ranks (K33)
    m.integrate(labels, poses[frame], weight=w); m.sample(poses[frame], own=labels, own_weight=w)   # a uint8 weight per voxel (visibility.py, K34)

The world lattice has the frame grid's voxel size; voxels live in 16^3 bricks of 16-bit vote counters, one row of `pitch`
= n_classes rounded up to 4 counters per voxel (8192 * pitch bytes per brick: 163840 at 20 classes).  The host side is
numpy in float64 and quantises to the int32 fixed point the kernel computes in (include/occdepth_amd.h).  The effect on
any score is not measured (no checkpoint and no dataset where this was built).
"""
import os

import numpy as np
import torch

from . import hip

BRICK = hip.MAP_BRICK
FRAC = 16                                   # fractional bits of the fixed point
C_LIMIT = float(1 << 14)                    # |c_k| below this: gq stays inside int32
KEY_BITS = 21                               # a key component lies in [-2^20, 2^20)
_KEY_OFF = 1 << (KEY_BITS - 1)
_SPHERE = 8.0 * np.sqrt(3.0) + 1.0          # a brick's bounding sphere about local (7.5, 7.5, 7.5), plus one voxel
_AXIS_MARGIN = 2.0 ** -8                    # voxels; the quantised transform is within 46 * 2^-17 of the exact one


# ----------------------------------------------------------------------------------------------------- geometry
def _pose(pose):
    pose = np.asarray(pose, dtype=np.float64)
    if pose.shape != (4, 4):
        raise ValueError("pose must be 4 x 4 (sensor -> world), got %r" % (pose.shape,))
    return pose[:3, :3], pose[:3, 3]


def _brick_offsets(pose, keys, vox_origin, voxel_size):
    """c_k = (R^T ((16 k + 1/2) v - t) - o) / v, (n, 3) float64: the grid coordinate of brick k's local voxel (0, 0, 0)."""
    R, t = _pose(pose)
    v = float(voxel_size)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    org = np.asarray(vox_origin, dtype=np.float64).reshape(3)
    world = (BRICK * keys.astype(np.float64) + 0.5) * v - t
    return (world @ R - org) / v            # rows of (R^T world^T)^T


def brick_coefficients(pose, keys, vox_origin, voxel_size):
    """-> Aq (3, 3) int32 = rint(R^T 2^16) and cq (n, 3) int32 = rint(c_k 2^16) for the bricks `keys` (n, 3): brick-local
    voxel (i, j, l) falls into the frame voxel (Aq (i, j, l) + cq) >> 16.  |c_k| >= 2^14 is refused."""
    R, _ = _pose(pose)
    c = _brick_offsets(pose, keys, vox_origin, voxel_size)
    if c.size and not np.abs(c).max() < C_LIMIT:
        raise ValueError("a brick lies %.0f voxels from the frame's grid origin: the fixed-point transform takes less "
                         "than 2^14 = %d" % (np.abs(c).max(), int(C_LIMIT)))
    scale = float(1 << FRAC)
    return np.rint(R.T * scale).astype(np.int32), np.rint(c * scale).astype(np.int32)


def frame_brick_box(pose, vox_origin, voxel_size, dims):
    """-> (lo, hi), int64 (3,): the inclusive brick-key box of the frame's candidate bricks, the brick range of the
    grid's eight corners in world voxels, one voxel wider on every side."""
    R, t = _pose(pose)
    v = float(voxel_size)
    dims = np.asarray(dims, dtype=np.float64).reshape(3)
    org = np.asarray(vox_origin, dtype=np.float64).reshape(3)
    corners = np.array([[x, y, z] for x in (0.0, dims[0]) for y in (0.0, dims[1]) for z in (0.0, dims[2])])
    world = ((corners * v + org) @ R.T + t) / v
    lo = np.floor((np.floor(world.min(0)) - 1.0) / BRICK).astype(np.int64)
    hi = np.floor((np.floor(world.max(0)) + 1.0) / BRICK).astype(np.int64)
    return lo, hi


def frame_bricks(pose, vox_origin, voxel_size, dims):
    """The keys (n, 3) int64, ascending, of every brick that can hold a voxel of the frame: the brick range of the
    grid's eight corners in world voxels, less the bricks whose bounding sphere (radius 8 sqrt 3, plus a voxel of margin)
    misses the grid box, less those whose extent along a grid axis misses it.  Over-selects; never drops a voting brick."""
    R, t = _pose(pose)
    dims = np.asarray(dims, dtype=np.float64).reshape(3)
    lo, hi = frame_brick_box(pose, vox_origin, voxel_size, dims)
    k0, k1, k2 = np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in range(3)), indexing="ij")
    keys = np.stack([k0, k1, k2], -1).reshape(-1, 3)                      # ascending (k0, k1, k2)
    centre = _brick_offsets(pose, keys, vox_origin, voxel_size) + 7.5 * R.T.sum(1)
    gap = np.maximum(np.maximum(-centre, centre - dims), 0.0)
    sphere = (gap * gap).sum(1) <= _SPHERE * _SPHERE
    # and along each grid axis the brick's voxel centres reach 7.5 sum_c |R^T[r][c]| from its centre; the margin covers the
    # fixed point's 3.5e-4 voxel with room to spare, and keeps a brick that merely touches the grid from the outside out
    reach = 7.5 * np.abs(R.T).sum(1) + _AXIS_MARGIN
    return keys[sphere & (gap <= reach).all(1)]


def sample_coefficients(pose, vox_origin, voxel_size, key_min, dims=None):
    """-> Bq (3, 3) int32 = rint(R 2^16) and dq (3,) int32 = rint(d 2^16), d = R (1/2 + o / v) + t / v - 16 key_min: the
    frame voxel (x, y, z) falls into the world voxel 16 key_min + ((Bq (x, y, z) + dq) >> 16) (occd_map_sample, K32).
    |d| >= 2^14 is refused, and with `dims` a grid of X + Y + Z >= 2^14: the fixed point stays inside int32."""
    R, t = _pose(pose)
    v = float(voxel_size)
    org = np.asarray(vox_origin, dtype=np.float64).reshape(3)
    W0 = BRICK * np.asarray(key_min, dtype=np.float64).reshape(3)
    if dims is not None and not sum(int(d) for d in dims) < int(C_LIMIT):
        raise ValueError("a frame of X + Y + Z = %d voxels: the fixed-point transform takes less than 2^14 = %d"
                         % (sum(int(d) for d in dims), int(C_LIMIT)))
    d = R @ (0.5 + org / v) + t / v - W0
    if not np.abs(d).max() < C_LIMIT:
        raise ValueError("the frame's grid origin lies %.0f voxels from its window's: the fixed-point transform takes less "
                         "than 2^14 = %d" % (np.abs(d).max(), int(C_LIMIT)))
    scale = float(1 << FRAC)
    return np.rint(R * scale).astype(np.int32), np.rint(d * scale).astype(np.int32)


def pack_keys(keys):
    """(n, 3) keys -> (n,) int64 whose order is the ascending (k0, k1, k2) order."""
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    if keys.size and (keys.min() < -_KEY_OFF or keys.max() >= _KEY_OFF):
        raise ValueError("brick keys must lie in [-2^20, 2^20)")
    k = keys + _KEY_OFF
    return (k[:, 0] << (2 * KEY_BITS)) | (k[:, 1] << KEY_BITS) | k[:, 2]


def unpack_keys(packed):
    p = np.asarray(packed, dtype=np.int64).reshape(-1)
    m = (1 << KEY_BITS) - 1
    return np.stack([p >> (2 * KEY_BITS), (p >> KEY_BITS) & m, p & m], -1) - _KEY_OFF


# ----------------------------------------------------------------------------------------------------- the map
class SemanticMap:
    """A growing sparse voxel map of vote counters.

    integrate() selects the bricks a frame can touch (frame_bricks), looks them up in the host directory {key -> pool
    slot}, gives new ones zeroed slots, and sends one table -- slot, key and the 12 fixed-point coefficients per brick --
    to the device in one asynchronous copy from a pinned buffer of its own (never one a copy in flight may still read),
    followed by one launch.  No host synchronisation, unless the pool has to grow.

    The pool `votes` is one (capacity, 16, 16, 16, pitch) int16 tensor holding uint16 bits.  The capacity is a multiple of
    `chunk_bricks`; when it runs out, the pool is reallocated and copied at the needed size rounded up to a chunk, and by
    at least half again, so the copies stay amortised.  `max_bricks` bounds it.  Over-selected bricks keep their slots
    (all zero).  At 20 classes a brick is 163840 bytes; a straight drive at 256 x 256 x 32 and a 45 degree heading adds
    2.72 MB of map per metre of new ground (profiles/map_ab.txt).
    """

    def __init__(self, n_classes, voxel_size, vox_origin, dims, max_bricks=None, chunk_bricks=1024):
        self.n_classes = int(n_classes)
        if not 1 <= self.n_classes <= 32:
            raise ValueError("1..32 classes, got %r" % (n_classes,))
        self.voxel_size = float(voxel_size)
        if not self.voxel_size > 0.0:
            raise ValueError("voxel_size must be positive, got %r" % (voxel_size,))
        self.vox_origin = tuple(float(x) for x in np.asarray(vox_origin, dtype=np.float64).reshape(3))
        self.dims = tuple(int(d) for d in dims)
        if len(self.dims) != 3 or min(self.dims) < 1 or self.dims[0] * self.dims[1] * self.dims[2] > 1 << 28:
            raise ValueError("dims must be (X, Y, Z) with X Y Z <= 2^28, got %r" % (dims,))
        self.chunk_bricks = int(chunk_bricks)
        self.max_bricks = None if max_bricks is None else int(max_bricks)
        if self.chunk_bricks < 1 or (self.max_bricks is not None and self.max_bricks < 1):
            raise ValueError("chunk_bricks and max_bricks must be >= 1")
        self.pitch = hip.round_up(self.n_classes, 4)
        self.brick_bytes = BRICK ** 3 * self.pitch * 2
        self.votes = None                   # (capacity, 16, 16, 16, pitch) int16, with the first integrate
        self.directory = {}                 # packed key -> slot
        self.grown = 0                      # pool (re)allocations so far

    # ------------------------------------------------------------------------------------------------ pool
    @property
    def n_bricks(self):
        return len(self.directory)

    @property
    def capacity(self):
        return 0 if self.votes is None else int(self.votes.shape[0])

    @property
    def nbytes(self):
        return self.capacity * self.brick_bytes

    def reset(self):
        """Forget every brick; the pool keeps its memory, zeroed."""
        self.directory = {}
        if self.votes is not None:
            self.votes.zero_()

    def release(self):
        """Forget every brick and give the pool's memory back."""
        self.directory = {}
        self.votes = None

    def pool(self):
        return self.votes.view(self.capacity, BRICK ** 3, self.pitch)

    def _reserve(self, need, device):
        if self.max_bricks is not None and need > self.max_bricks:
            raise RuntimeError("the map needs %d bricks, max_bricks = %d allows %.1f MB of vote counters (%d bytes per "
                               "brick at %d classes)" % (need, self.max_bricks, self.max_bricks * self.brick_bytes / 1e6,
                                                         self.brick_bytes, self.n_classes))
        cap = self.capacity
        if need <= cap:
            return
        new_cap = hip.round_up(max(need, cap + cap // 2), self.chunk_bricks)
        if self.max_bricks is not None:
            new_cap = min(new_cap, self.max_bricks)
        votes = torch.zeros((new_cap, BRICK, BRICK, BRICK, self.pitch), dtype=torch.int16, device=device)
        if cap:
            votes[:cap].copy_(self.votes)
        self.votes = votes
        self.grown += 1

    def slots(self, keys, create=False, device=None):
        """(n, 3) keys -> (n,) int32 pool slots, -1 for a key that is not in the map (create: it takes the next slot)."""
        packed = pack_keys(keys).tolist()
        d = self.directory
        out = [d.get(p, -1) for p in packed]
        if create:
            new = [i for i, s in enumerate(out) if s < 0]
            if new:
                self._reserve(len(d) + len(new), device)
                for i in new:
                    out[i] = d[packed[i]] = len(d)
        return np.asarray(out, dtype=np.int32).reshape(-1)

    def upload(self, table, device):
        """One table -> (device copy, host copy).  On a GPU the host copy is a fresh pinned tensor: the caching host
        allocator hands its memory out again only after the asynchronous copy that reads it has run."""
        host = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32))
        if torch.device(device).type != "cuda":
            return host, host
        host = host.pin_memory()
        return host.to(device, non_blocking=True), host

    # ------------------------------------------------------------------------------------------------ integrate
    def frame_table(self, pose, device):
        """The (n, 16) int32 launch table of one frame -- slot | key | Aq | cq per brick -- with new bricks admitted."""
        keys = frame_bricks(pose, self.vox_origin, self.voxel_size, self.dims)
        Aq, cq = brick_coefficients(pose, keys, self.vox_origin, self.voxel_size)
        table = np.empty((len(keys), 16), dtype=np.int32)
        table[:, 0] = self.slots(keys, create=True, device=device)
        table[:, 1:4] = keys
        table[:, 4:13] = Aq.reshape(9)
        table[:, 13:16] = cq
        return table

    def _weight(self, weight, device, name):
        """A weight volume as the weighted kernels take it: X Y Z uint8 entries on `device`."""
        weight = torch.as_tensor(weight)
        S = self.dims[0] * self.dims[1] * self.dims[2]
        if weight.dtype != torch.uint8 or weight.numel() != S:
            raise ValueError("%s must hold X Y Z = %d uint8 weights (visibility.vote_weights), got %s %r"
                             % (name, S, weight.dtype, tuple(weight.shape)))
        return weight.to(device).contiguous()

    def integrate(self, labels, pose, mask=None, weight=None):
        """One frame votes: labels (X, Y, Z) uint8 / int16 (uint16 bits) on the GPU, pose 4 x 4 sensor -> world, mask the
        frame's own (X Y Z) bool / uint8 table or None.  A label >= n_classes (255) does not vote.  weight: instead of a
        mask (a frame takes one or the other), the (X Y Z) uint8 weight of each voxel's vote, 0 = no vote
        (visibility.vote_weights); counters saturate at 65535 either way, and frames of both kinds may share a map."""
        if tuple(labels.shape) != self.dims:
            raise ValueError("integrate takes (X, Y, Z) = %r labels, got %r" % (self.dims, tuple(labels.shape)))
        if self.votes is not None and labels.device != self.votes.device:
            raise ValueError("labels are on %s, the map on %s" % (labels.device, self.votes.device))
        if mask is not None and weight is not None:
            raise ValueError("a frame votes inside a mask or with a weight per voxel, not both (a weight of 0 is the mask)")
        if weight is not None:
            weight = self._weight(weight, labels.device, "weight")
        S = self.dims[0] * self.dims[1] * self.dims[2]
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.numel() != S:
                raise ValueError("mask must hold X Y Z = %d entries, got %r" % (S, tuple(mask.shape)))
            mask = mask.to(labels.device)
            if mask.dtype not in (torch.bool, torch.uint8):
                mask = mask != 0
        table = self.frame_table(pose, labels.device)
        if not len(table):
            return self
        dev_table, host_table = self.upload(table, labels.device)
        if weight is not None:
            hip.map_integrate_weighted(self.pool(), dev_table, labels.contiguous(), self.dims, self.n_classes, weight,
                                       table_host=host_table)
            return self
        hip.map_integrate(self.pool(), dev_table, labels.contiguous(), self.dims, self.n_classes, mask=mask,
                          table_host=host_table)
        return self

    # ------------------------------------------------------------------------------------------------ read-back
    def frame_cells(self, pose, device):
        """The window of one frame for sample() -> (cells, table, key_min): the inclusive brick-key box of the frame's
        candidates (frame_brick_box; every brick of the box, not only those frame_bricks keeps), table (n, 16) int32 in
        integrate's layout -- slot | key | Aq | cq -- for the n bricks of the box that the map holds (none is admitted,
        the pool never grows), and cells (gx, gy, gz) int32, the table row of the brick at each cell or -1.  Both are
        numpy arrays; `device` is where they will go (kept for symmetry with frame_table)."""
        lo, hi = frame_brick_box(pose, self.vox_origin, self.voxel_size, self.dims)
        grid = tuple(int(g) for g in hi - lo + 1)
        k0, k1, k2 = np.meshgrid(*(np.arange(lo[a], hi[a] + 1) for a in range(3)), indexing="ij")
        keys = np.stack([k0, k1, k2], -1).reshape(-1, 3)
        slots = self.slots(keys, create=False)
        have = slots >= 0
        keys = keys[have]
        Aq, cq = brick_coefficients(pose, keys, self.vox_origin, self.voxel_size)
        table = np.empty((len(keys), 16), dtype=np.int32)
        table[:, 0] = slots[have]
        table[:, 1:4] = keys
        table[:, 4:13] = Aq.reshape(9)
        table[:, 13:16] = cq
        cells = np.full(grid, -1, dtype=np.int32)
        at = keys - lo
        cells[at[:, 0], at[:, 1], at[:, 2]] = np.arange(len(keys), dtype=np.int32)
        return cells, table, lo

    def sample(self, pose, own=None, own_mask=None, min_obs=1, exclude_self=False, keep_own=False, own_weight=None):
        """What the whole map says about the voxels of the frame at `pose` (K32, one launch) -> labels (X, Y, Z) uint8,
        n_obs (X, Y, Z) int16 holding uint16 bits (the votes at the world voxel the frame voxel's centre falls into,
        saturated at 65535).  labels = the arg-max of those votes (the lowest class on a tie) where n_obs >= max(min_obs,
        1); elsewhere `own` (the frame's own labels, (X, Y, Z) uint8 / int16 on the map's device; >= 255 -> 255) when
        given, else 255.  exclude_self takes the frame's own vote out first: `own` and `own_mask` must be what it was
        integrated with (a counter saturated at 65535 is not retracted).  keep_own: a tie that own's class is part of
        goes to own.  An empty map, or a frame that meets none of its bricks, gives the fallback volume and zeros
        without a launch.  own_weight (instead of own_mask, never both): the (X Y Z) uint8 weights the frame was
        integrated with; exclude_self then retracts that weight (not from a counter saturated at 65535, nor from one
        below the weight), and n_obs and min_obs count vote units, as they do for any map that took weighted votes."""
        if int(min_obs) < 0:
            raise ValueError("min_obs must be >= 0, got %r" % (min_obs,))
        if own_mask is not None and own_weight is not None:
            raise ValueError("a frame voted inside own_mask or with own_weight, not both")
        if own is None and (exclude_self or keep_own):
            raise ValueError("exclude_self and keep_own need the frame's own labels (own)")
        if not sum(self.dims) < int(C_LIMIT):
            raise ValueError("a frame of X + Y + Z = %d voxels: the fixed-point transform takes less than 2^14" % sum(self.dims))
        dev = self.votes.device if self.votes is not None else (own.device if own is not None else torch.device("cpu"))
        S = self.dims[0] * self.dims[1] * self.dims[2]
        if own is not None:
            if tuple(own.shape) != self.dims:
                raise ValueError("sample takes own (X, Y, Z) = %r labels, got %r" % (self.dims, tuple(own.shape)))
            if own.device != dev:
                raise ValueError("own is on %s, the map on %s" % (own.device, dev))
        if own_mask is not None:
            own_mask = torch.as_tensor(own_mask)
            if own_mask.numel() != S:
                raise ValueError("own_mask must hold X Y Z = %d entries, got %r" % (S, tuple(own_mask.shape)))
            own_mask = own_mask.to(dev)
            if own_mask.dtype not in (torch.bool, torch.uint8):
                own_mask = own_mask != 0
        if own_weight is not None:
            own_weight = self._weight(own_weight, dev, "own_weight")
        table = None
        if self.votes is not None and self.directory:
            cells, table, key_min = self.frame_cells(pose, dev)
        if table is None or not len(table):
            if own is None:
                labels = torch.full(self.dims, 255, dtype=torch.uint8, device=dev)
            else:
                wide = own.to(torch.int32) & 0xFFFF
                labels = torch.where(wide < 255, wide, torch.full_like(wide, 255)).to(torch.uint8)
            return labels, torch.zeros(self.dims, dtype=torch.int16, device=dev)
        Bq, dq = sample_coefficients(pose, self.vox_origin, self.voxel_size, key_min, self.dims)
        dev_table, host_table = self.upload(table, dev)
        dev_cells, _ = self.upload(cells, dev)
        if own_weight is not None:
            return hip.map_sample_weighted(self.pool(), dev_table, dev_cells, None if own is None else own.contiguous(),
                                           self.dims, self.n_classes, Bq, dq, cells.shape, own_weight=own_weight,
                                           min_obs=int(min_obs), exclude_self=bool(exclude_self), keep_own=bool(keep_own),
                                           table_host=host_table)
        return hip.map_sample(self.pool(), dev_table, dev_cells, None if own is None else own.contiguous(), self.dims,
                              self.n_classes, Bq, dq, cells.shape, own_mask=own_mask, min_obs=int(min_obs),
                              exclude_self=bool(exclude_self), keep_own=bool(keep_own), table_host=host_table)

    # ------------------------------------------------------------------------------------------------ extraction
    def brick_keys(self):
        """The keys of the map's bricks, (n, 3) int64, ascending (k0, k1, k2)."""
        return unpack_keys(np.sort(np.fromiter(self.directory.keys(), dtype=np.int64, count=len(self.directory))))

    def _key_table(self, keys):
        keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
        table = np.empty((len(keys), 4), dtype=np.int32)
        table[:, 0] = self.slots(keys)
        table[:, 1:4] = keys
        return table

    def brick_labels(self, keys, device=None):
        """(n, 3) keys -> (n, 16, 16, 16) uint8 labels (argmax of the votes, the lowest class on a tie), 255 where a voxel
        has no vote or the key is not in the map."""
        table = self._key_table(keys)
        if self.votes is None or not len(table):
            return torch.full((len(table), BRICK, BRICK, BRICK), 255, dtype=torch.uint8,
                              device=self.votes.device if self.votes is not None else (device or "cpu"))
        dev_table, host_table = self.upload(table, self.votes.device)
        return hip.map_brick_labels(self.pool(), dev_table, self.n_classes, table_host=host_table)

    def extract(self, min_obs=1, include_empty=False):
        """The voxels with at least `min_obs` votes (and a label other than 0, empty, unless include_empty) -> coords
        (N, 3) int32 world voxel indices, labels (N,) uint8, n_obs (N,) int16 holding uint16 bits (the votes, saturated
        at 65535).  Bricks by ascending key, voxels inside a brick in (i, j, l) order: the same bits on every run."""
        if int(min_obs) < 0:
            raise ValueError("min_obs must be >= 0, got %r" % (min_obs,))
        if self.votes is None or not self.directory:
            dev = self.votes.device if self.votes is not None else "cpu"
            return (torch.empty((0, 3), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.uint8, device=dev),
                    torch.empty((0,), dtype=torch.int16, device=dev))
        dev_table, host_table = self.upload(self._key_table(self.brick_keys()), self.votes.device)
        return hip.map_extract(self.pool(), dev_table, self.n_classes, min_obs=min_obs, include_empty=include_empty,
                               table_host=host_table)


    # ------------------------------------------------------------------------------------------------ merge (K33)
    def occupied_keys(self, chunk_bricks=512):
        """The keys, (n, 3) int64 ascending, of the bricks that hold at least one vote: frame_bricks over-selects, and
        an all-zero brick need neither travel nor be written.  Torch operators on the pool; one host synchronisation."""
        keys = self.brick_keys()
        if not len(keys):
            return keys
        slots = torch.from_numpy(self.slots(keys).astype(np.int64)).to(self.votes.device)
        words = self.pool().view(self.capacity, -1).view(torch.int64)       # a brick is 2048 * pitch 8-byte words
        flags = [words.index_select(0, slots[s:s + int(chunk_bricks)]).ne(0).any(1)
                 for s in range(0, len(keys), int(chunk_bricks))]
        return keys[torch.cat(flags).cpu().numpy()]

    def _merge_from(self, keys, src, src_rows, device):
        """votes[slot of keys[i]] += src[src_rows[i]], saturating; keys the map lacks are admitted in ascending order."""
        keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
        packed = pack_keys(keys)
        if len(np.unique(packed)) != len(packed):
            raise ValueError("merge_rows takes every brick key once: %d of %d keys are repeats"
                             % (len(packed) - len(np.unique(packed)), len(packed)))
        if not len(keys):
            return self
        new = np.sort(np.fromiter((p for p in packed.tolist() if p not in self.directory), dtype=np.int64))
        if len(new):
            self.slots(unpack_keys(new), create=True, device=device)       # refuses before it changes anything
        table = np.stack([self.slots(keys), np.asarray(src_rows, dtype=np.int32).reshape(-1)], 1)
        dev_table, host_table = self.upload(table, self.votes.device)
        hip.map_merge(self.pool(), src, dev_table, table_host=host_table)
        return self

    def merge_rows(self, keys, rows, device=None):
        """Add bricks of counters to the map (K33, one launch): keys (n, 3) int64, each once; rows (n, 4096, pitch)
        int16 holding uint16 bits, row i the brick keys[i] -- used as it is on the map's device, copied there from
        anywhere else (an empty map takes `device`, else the rows' device).  votes = min(votes + rows, 65535).  Keys the
        map lacks are admitted, new bricks taking slots in ascending key order.  No host synchronisation unless the pool
        has to grow; max_bricks is checked before anything changes."""
        rows = torch.as_tensor(rows)
        keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
        if rows.dtype != torch.int16 or tuple(rows.shape) != (len(keys), BRICK ** 3, self.pitch):
            raise ValueError("merge_rows takes int16 rows (%d, %d, %d) for its %d keys, got %s %r"
                             % (len(keys), BRICK ** 3, self.pitch, len(keys), rows.dtype, tuple(rows.shape)))
        dev = self.votes.device if self.votes is not None else torch.device(device if device is not None else rows.device)
        if rows.device != dev:
            rows = rows.to(dev)                                             # blocking: the caller may reuse its buffer
        return self._merge_from(keys, rows.contiguous(), np.arange(len(keys)), dev)

    def merge(self, other):
        """Add another map's votes to this one: the map of a set of frames is the counter-wise saturating sum of the
        maps of any partition of the set.  One launch straight from other.pool(), without a copy when both maps share a
        device.  n_classes and voxel_size must agree; vox_origin and dims may differ: they describe the frames a map
        integrates, not the world lattice, which the voxel size alone fixes.  An empty `other` changes nothing."""
        if other is self:
            raise ValueError("a map cannot be merged into itself (every counter would have two owners)")
        if other.n_classes != self.n_classes or other.voxel_size != self.voxel_size:
            raise ValueError("the maps differ in classes (%d, %d) or voxel size (%r, %r): their counters or lattices differ"
                             % (self.n_classes, other.n_classes, self.voxel_size, other.voxel_size))
        if other.votes is None or not other.directory:
            return self
        keys = other.brick_keys()
        rows = other.slots(keys)
        dev = self.votes.device if self.votes is not None else other.votes.device
        src = other.pool()
        if src.device != dev:
            src = src[:other.n_bricks].to(dev)                              # only the bricks in use travel; slots are 0 .. n - 1
        return self._merge_from(keys, src, rows, dev)

    # ------------------------------------------------------------------------------------------------ save / load
    def _staging(self, chunk, device):
        buf = torch.empty((chunk, BRICK ** 3, self.pitch), dtype=torch.int16)
        return buf.pin_memory() if torch.device(device).type == "cuda" else buf

    def save(self, path, chunk_bricks=None):
        """Write the occupied bricks to `path` (the .occmap format): MAP_MAGIC, the header MAP_HEADER,
        the keys (n, 3) little-endian int32 ascending, then the n bricks' counter rows in that order.  The rows pass
        through one pinned buffer of `chunk_bricks` bricks (default: the map's): the map never needs a host copy.  -> path."""
        keys = self.occupied_keys()
        chunk = max(1, int(chunk_bricks or self.chunk_bricks))
        header = np.zeros((), dtype=MAP_HEADER)
        header["n_classes"], header["pitch"], header["brick"] = self.n_classes, self.pitch, BRICK
        header["voxel_size"], header["vox_origin"], header["dims"] = self.voxel_size, self.vox_origin, self.dims
        header["n_bricks"] = len(keys)
        with open(path, "wb") as f:
            f.write(MAP_MAGIC)
            f.write(header.tobytes())
            f.write(keys.astype("<i4").tobytes())
            if len(keys):
                dev = self.votes.device
                slots = torch.from_numpy(self.slots(keys).astype(np.int64)).to(dev)
                buf = self._staging(min(chunk, len(keys)), dev)
                for s in range(0, len(keys), chunk):
                    part = buf[:len(slots[s:s + chunk])]
                    part.copy_(self.pool().index_select(0, slots[s:s + chunk]))          # blocking
                    f.write(memoryview(part.numpy()).cast("B"))
        return path

    @classmethod
    def load(cls, path, device=None, max_bricks=None, chunk_bricks=None):
        """A file save() wrote -> a new map on `device` (default: the GPU when there is one) holding its bricks, in
        slots 0 .. n - 1 by ascending key.  Read `chunk_bricks` bricks at a time through one pinned buffer.  Refuses a
        wrong magic or version, a brick edge other than this build's, and a file whose length disagrees with its header."""
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            magic = f.read(len(MAP_MAGIC))
            if magic != MAP_MAGIC:
                raise ValueError("%s is not an occdepth_amd map file of this version: it starts with %r, not %r"
                                 % (path, magic, MAP_MAGIC))
            raw = f.read(MAP_HEADER.itemsize)
            if len(raw) != MAP_HEADER.itemsize:
                raise ValueError("%s: %d bytes, its header alone takes %d" % (path, size, len(MAP_MAGIC) + MAP_HEADER.itemsize))
            h = np.frombuffer(raw, dtype=MAP_HEADER)[0]
            if int(h["brick"]) != BRICK:
                raise ValueError("%s holds bricks of edge %d, this build has %d" % (path, int(h["brick"]), BRICK))
            n, pitch = int(h["n_bricks"]), int(h["pitch"])
            m = cls(int(h["n_classes"]), float(h["voxel_size"]), tuple(h["vox_origin"].tolist()), tuple(h["dims"].tolist()),
                    max_bricks=max_bricks, **({} if chunk_bricks is None else {"chunk_bricks": int(chunk_bricks)}))
            if n < 0 or pitch != m.pitch:
                raise ValueError("%s: a header of %d bricks at pitch %d for %d classes" % (path, n, pitch, m.n_classes))
            want = len(MAP_MAGIC) + MAP_HEADER.itemsize + n * (12 + m.brick_bytes)
            if size != want:
                raise ValueError("%s: %d bytes, its header announces %d" % (path, size, want))
            keys = np.frombuffer(f.read(12 * n), dtype="<i4").reshape(n, 3).astype(np.int64)
            if n and (np.diff(pack_keys(keys)) <= 0).any():
                raise ValueError("%s: its brick keys are not ascending" % path)
            if not n:
                return m
            dev = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
            slots = m.slots(keys, create=True, device=dev)                  # 0 .. n - 1; max_bricks refuses here
            buf = m._staging(min(m.chunk_bricks, n), dev)
            for s in range(0, n, m.chunk_bricks):
                part = buf[:len(slots[s:s + m.chunk_bricks])]
                f.readinto(memoryview(part.numpy()).cast("B"))
                m.pool()[s:s + len(part)].copy_(part)                       # blocking: the buffer is read into again
        return m


MAP_MAGIC = b"OCCDMAP1"                     # the last byte is the format version
MAP_HEADER = np.dtype([("n_classes", "<i4"), ("pitch", "<i4"), ("brick", "<i4"), ("reserved", "<i4"), ("voxel_size", "<f8"),
                       ("vox_origin", "<f8", (3,)), ("dims", "<i4", (3,)), ("reserved2", "<i4"), ("n_bricks", "<i8")])


def merge_over_ranks(m, group=None, chunk_bricks=256, device=None):
    """A collective over a torch.distributed group: leaves on every rank the same map, counter for counter -- the sum of
    all ranks' maps.  The ranks exchange their occupied_keys(), admit the union in ascending order (so the directories
    agree too), and for source rank r = 0 .. W - 1 the rows of r's bricks are broadcast `chunk_bricks` at a time and
    merged (merge_rows) by every other rank.  The buffer lives on the device when the backend moves device tensors
    (RCCL, which torch calls nccl), else in pinned host memory (gloo).  A rank other than the first keeps a copy of its
    own occupied rows from before the first merge: what it sends must not hold what it received.  Each rank receives
    W - 1 maps' worth of rows.  All ranks must agree on n_classes, pitch and voxel_size.  A world of one, or no
    process group, returns at once.  An empty map takes `device` (default: the current GPU when there is one)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return m
    W = dist.get_world_size(group)
    if W < 2:
        return m
    rank = dist.get_rank(group)
    chunk = max(1, int(chunk_bricks))
    mine = pack_keys(m.occupied_keys())
    shape = (m.n_classes, m.pitch, m.voxel_size)
    said = [None] * W
    dist.all_gather_object(said, (shape, mine), group=group)
    if any(s[0] != shape for s in said):
        raise ValueError("the ranks' maps differ in (n_classes, pitch, voxel_size): %r" % ([s[0] for s in said],))
    union = np.unique(np.concatenate([s[1] for s in said]))
    if not len(union):
        return m
    dev = m.votes.device if m.votes is not None else torch.device(
        device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
    m.slots(unpack_keys(union), create=True, device=dev)
    on_device = dist.get_backend(group) == "nccl" and dev.type == "cuda"
    n_max = max(len(s[1]) for s in said)
    buf = (torch.empty((min(chunk, n_max), BRICK ** 3, m.pitch), dtype=torch.int16, device=dev) if on_device
           else m._staging(min(chunk, n_max), dev))
    own_slots = torch.from_numpy(m.slots(unpack_keys(mine)).astype(np.int64)).to(dev)
    own = None
    if rank > 0 and len(mine):                                              # rank 0 has sent before it merges
        own = m.pool().index_select(0, own_slots) if on_device else torch.cat(
            [m.pool().index_select(0, own_slots[s:s + chunk]).cpu() for s in range(0, len(mine), chunk)])
    for r in range(W):
        keys_r = said[r][1]
        src = dist.get_global_rank(group, r) if group is not None else r
        for s in range(0, len(keys_r), chunk):
            part = buf[:len(keys_r[s:s + chunk])]
            if r == rank:
                part.copy_(m.pool().index_select(0, own_slots[s:s + chunk]) if own is None else own[s:s + len(part)])
            dist.broadcast(part.view(torch.int32), src, group=group)       # gloo moves no 16-bit integers
            if r != rank:
                m.merge_rows(unpack_keys(keys_r[s:s + chunk]), part)
    return m


def map_confusion(pred_map, gt_map, metric, chunk_bricks=512):
    """Count the prediction map against the ground-truth map into `metric` (SSCMetrics.add_batch): the ground-truth
    map's bricks in chunks, both maps' dense labels, the target set to 255 where the prediction is unobserved -- a voxel
    counts only where both maps were observed."""
    if pred_map.voxel_size != gt_map.voxel_size:
        raise ValueError("the two maps have different voxel sizes (%r, %r): their lattices differ"
                         % (pred_map.voxel_size, gt_map.voxel_size))
    keys = gt_map.brick_keys()
    dev = gt_map.votes.device if gt_map.votes is not None else None
    for s in range(0, len(keys), int(chunk_bricks)):
        part = keys[s:s + int(chunk_bricks)]
        target = gt_map.brick_labels(part)
        pred = pred_map.brick_labels(part, device=dev)
        metric.add_batch(pred, torch.where(pred == 255, pred, target))
    return metric


# ----------------------------------------------------------------------------------------------------- drawable form
MAX_CELLS = 1 << 27                         # directory entries of a MapVolume (512 MB of int32)
MAX_GRID = 1 << 16                          # bricks along one axis of its window


class MapVolume:
    """A map in the form render.render_map draws (K31, csrc/map_render.hip): one 4096-byte row of labels per brick and a
    dense directory of the bricks over the map's bounding window.

    Rows: the brick keys of `pred`, united with those of `gt` when given, clipped to the inclusive brick-key box
    key_range = (lo(3), hi(3)) when given, ascending in (k0, k1, k2).  labels (n, 4096) uint8 = pred.brick_labels(keys),
    with min_obs > 1 set to 255 where a voxel has fewer votes; target (n, 4096) uint8 = gt.brick_labels(keys), set to 255
    where the prediction is 255 (map_confusion's rule: a voxel counts only where both maps were observed), or None.
    Window: key_min / key_max over the rows, grid = key_max - key_min + 1 bricks, dims = 16 grid voxels, origin_voxels =
    16 key_min (int64), origin_metres = origin_voxels * voxel_size (float64); world voxel I spans [I v, (I + 1) v).
    Directory: cells (Gx, Gy, Gz) int32 on the device, the row of the brick at that cell, -1 where there is none and,
    with drop_empty, where the brick holds no drawable voxel (its row stays: row indices are stable).  Drawable: label in
    1..254 (what class mode draws); with a target also target != 255 and (label in 1..254 or target != 0) (what error mode
    draws, and a class-mode picture of the target) -- a brick is dropped only when no mode would draw any of its voxels,
    so one volume serves the prediction, ground-truth and error pictures.  No host synchronisation.

        def target_volume(): the same window with the target as labels (the ground-truth picture)."""

    def __init__(self, pred, gt=None, min_obs=1, key_range=None, drop_empty=True, chunk_bricks=512):
        if gt is not None and (pred.voxel_size != gt.voxel_size or pred.n_classes != gt.n_classes):
            raise ValueError("the two maps differ in voxel size (%r, %r) or classes (%r, %r)"
                             % (pred.voxel_size, gt.voxel_size, pred.n_classes, gt.n_classes))
        if int(min_obs) < 1:
            raise ValueError("min_obs must be >= 1, got %r" % (min_obs,))
        self.voxel_size, self.n_classes, self.min_obs = pred.voxel_size, pred.n_classes, int(min_obs)
        packed = set(pred.directory) | (set(gt.directory) if gt is not None else set())
        keys = unpack_keys(np.sort(np.fromiter(packed, dtype=np.int64, count=len(packed))))
        if key_range is not None:
            lo, hi = (np.asarray(k, dtype=np.int64).reshape(3) for k in key_range)
            keys = keys[((keys >= lo) & (keys <= hi)).all(1)]
        if not len(keys):
            raise ValueError("the map has no brick to draw" + ("" if key_range is None else " inside key_range = %r" % (key_range,))
                             + " (key_range selects an inclusive box of brick keys)")
        self.keys = keys
        self.key_min, self.key_max = keys.min(0), keys.max(0)
        grid = self.key_max - self.key_min + 1
        if grid.max() > MAX_GRID or int(grid[0]) * int(grid[1]) * int(grid[2]) > MAX_CELLS:
            raise ValueError("the map's window is %d x %d x %d bricks: more than 2^16 along an axis or more than 2^27 cells; "
                             "draw a part of it with key_range" % tuple(grid))
        self.grid = tuple(int(g) for g in grid)
        self.dims = tuple(BRICK * g for g in self.grid)
        self.origin_voxels = BRICK * self.key_min
        self.origin_metres = self.origin_voxels.astype(np.float64) * self.voxel_size
        dev = next((m.votes.device for m in (pred, gt) if m is not None and m.votes is not None), torch.device("cpu"))
        labels, target, drawn = [], [], []
        for s in range(0, len(keys), int(chunk_bricks)):
            part = keys[s:s + int(chunk_bricks)]
            lab = pred.brick_labels(part, device=dev).reshape(len(part), BRICK ** 3)
            if self.min_obs > 1 and pred.votes is not None:
                slots = torch.from_numpy(pred.slots(part).astype(np.int64))
                have = slots >= 0
                n_obs = torch.zeros(lab.shape, dtype=torch.int32, device=dev)
                if bool(have.any()):
                    votes = pred.pool()[slots[have].to(dev)]
                    n_obs[have.to(dev)] = (votes.to(torch.int32) & 0xFFFF).sum(-1, dtype=torch.int32)
                lab = torch.where(n_obs < self.min_obs, torch.full_like(lab, 255), lab)
            occ = (lab > 0) & (lab < 255)
            if gt is not None:
                tg = gt.brick_labels(part, device=dev).reshape(len(part), BRICK ** 3)
                tg = torch.where(lab == 255, lab, tg)
                target.append(tg)
                occ = occ | ((tg != 255) & (tg != 0))                       # class mode's rule or error mode's
            labels.append(lab)
            drawn.append(occ.any(1))
        self.labels = torch.cat(labels).contiguous()
        self.target = torch.cat(target).contiguous() if gt is not None else None
        self.drawable = torch.cat(drawn)                                     # (n,) bool: the brick holds something to draw
        rows = torch.arange(len(keys), dtype=torch.int32, device=dev)
        if drop_empty:
            rows = torch.where(self.drawable, rows, torch.full_like(rows, -1))
        at = torch.from_numpy(keys - self.key_min).to(dev)
        self.cells = torch.full(self.grid, -1, dtype=torch.int32, device=dev)
        self.cells[at[:, 0], at[:, 1], at[:, 2]] = rows

    def target_volume(self):
        """The same rows and directory with the target as labels and no target: class mode draws the ground truth."""
        if self.target is None:
            raise ValueError("the volume was built without a ground-truth map")
        import copy
        v = copy.copy(self)
        v.labels, v.target = self.target, None
        return v

    @property
    def n_rows(self):
        return int(self.labels.shape[0])

    @property
    def device(self):
        return self.labels.device


# ----------------------------------------------------------------------------------------------------- PLY
PLY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                      ("label", "u1"), ("n_obs", "<u2")])
_PLY_PROPS = ("float x", "float y", "float z", "uchar red", "uchar green", "uchar blue", "uchar label", "ushort n_obs")


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def write_ply(path, coords, labels, n_obs, voxel_size, colours):
    """A binary little-endian point PLY, one vertex per voxel: x y z float32 (the voxel centre in world metres),
    red green blue uchar (colours[label]; render.palette), label uchar, n_obs ushort.  -> path."""
    coords = _host(coords).reshape(-1, 3).astype(np.int64)
    labels = _host(labels).reshape(-1).astype(np.uint8)
    n_obs = _host(n_obs).reshape(-1).astype(np.int64) & 0xFFFF
    colours = _host(colours).reshape(-1, 3).astype(np.uint8)
    if not (len(coords) == len(labels) == len(n_obs)):
        raise ValueError("coords, labels and n_obs must have one entry per voxel")
    if len(labels) and int(labels.max()) >= len(colours):
        raise ValueError("label %d has no colour (%d rows)" % (int(labels.max()), len(colours)))
    rows = np.empty(len(labels), dtype=PLY_DTYPE)
    centre = (coords.astype(np.float64) + 0.5) * float(voxel_size)
    rows["x"], rows["y"], rows["z"] = centre[:, 0], centre[:, 1], centre[:, 2]
    rgb = colours[labels]
    rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    rows["label"], rows["n_obs"] = labels, n_obs
    header = ["ply", "format binary_little_endian 1.0", "comment occdepth_amd semantic map voxel_size %r" % float(voxel_size),
              "element vertex %d" % len(rows)] + ["property " + p for p in _PLY_PROPS] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rows.tobytes())
    return path


def read_ply(path):
    """A file write_ply wrote -> {"x", "y", "z", "red", "green", "blue", "label", "n_obs"} as one structured array, plus
    the voxel size of its comment line (None without one): (vertices, voxel_size)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError("%s is not a PLY file" % path)
    lines = data[:end].decode("ascii").splitlines()
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError("%s: only binary_little_endian 1.0 is read, got %r" % (path, lines[1]))
    count = voxel_size = None
    props = []
    for line in lines[2:]:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            count = int(w[2])
        elif w[0] == "property":
            props.append(" ".join(w[1:]))
        elif w[0] == "comment" and "voxel_size" in w:
            voxel_size = float(w[w.index("voxel_size") + 1])
    if count is None or tuple(props) != _PLY_PROPS:
        raise ValueError("%s does not have the vertex layout write_ply writes" % path)
    body = data[end + len(b"end_header\n"):]
    if len(body) != count * PLY_DTYPE.itemsize:
        raise ValueError("%s: %d bytes of vertices, its header announces %d" % (path, len(body), count * PLY_DTYPE.itemsize))
    return np.frombuffer(body, dtype=PLY_DTYPE), voxel_size
