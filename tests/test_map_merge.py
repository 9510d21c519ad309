"""CPU: the sum of maps (K33) -- SemanticMap.merge / merge_rows / occupied_keys, save and load, merge_over_ranks over two
gloo ranks, the model hook under two ranks and the offline tool's --save-map / --load-map, with the kernels replaced by
the stand-in of tests/test_map.py plus a numpy `merge`; and the argument checks of occd_map_merge before any launch.
Every comparison is exact integer equality against the map of all frames and against `MapRef`."""
import ctypes
import datetime
import functools
import os
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from occdepth_amd import hip
from occdepth_amd import semantic_map as sm
from test_map import (B, GRIDS, HOOK_C, V, KernelStandIn, MapRef, _confusion_stand_in, _epoch, _hook_steps, _hook_stub,
                      _tool, _write_sequence, assert_map_equals_ref, frames_for, sequence)
from test_map_gpu import CASES, IDS
from test_map_sample import SampleStandIn, _hook_world
from test_shard_gloo import _free_port


class MergeStandIn(KernelStandIn):
    """The stand-in of tests/test_map.py plus hip.map_merge in numpy: dst = min(dst + src, 65535) per table row."""

    NAMES = (("map_integrate", "integrate"), ("map_brick_labels", "brick_labels"), ("map_extract", "extract"), ("map_merge", "merge"))

    def install(self, monkeypatch):
        super().install(monkeypatch)
        monkeypatch.setattr(hip, "map_merge", self.merge)
        return self

    def install_in_process(self):
        """For a spawned rank, which has no monkeypatch and ends with its process."""
        for name, method in self.NAMES:
            setattr(hip, name, getattr(self, method))
        return self

    def merge(self, votes, src, table, table_host=None, split=0):
        v, s, t = self._u16(votes), self._u16(src), table.numpy().astype(np.int64)
        assert t.shape[1] == 2 and len(set(t[:, 0].tolist())) == len(t) and v.shape[2] == s.shape[2]
        assert t[:, 0].min() >= 0 and t[:, 0].max() < len(v) and t[:, 1].min() >= 0 and t[:, 1].max() < len(s)
        assert table_host is not None and torch.equal(table_host, table)
        assert not np.shares_memory(v, s)
        self.calls.append({"merge": len(t)})
        for slot, row in t:
            v[slot] = np.minimum(v[slot].astype(np.int64) + s[row].astype(np.int64), 65535).astype(np.uint16)
        return votes


def _cpu(lab):
    return torch.from_numpy(lab if lab.dtype == np.uint8 else lab.view(np.int16))


def case_frames(case):
    dims, C, label_bytes, masked = case
    return frames_for(dims, C, 100 * C + label_bytes, 6, label_bytes, masked), sequence(dims)


def build(case, which, chunk=8, **kw):
    """The map of the frames `which` of the case's six, on the CPU through the installed stand-in."""
    dims, C = case[0], case[1]
    frames, poses = case_frames(case)
    m = sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=chunk, **kw)
    for i in which:
        lab, mask = frames[i]
        m.integrate(_cpu(lab), poses[i], mask=None if mask is None else torch.from_numpy(mask))
    return m


@functools.lru_cache(maxsize=None)
def restatement(case):
    dims, C = case[0], case[1]
    frames, poses = case_frames(case)
    ref = MapRef(C, GRIDS[dims], dims)
    for (lab, mask), P in zip(frames, poses):
        ref.integrate(lab, P, mask)
    return ref


def counters(m):
    """{key: (4096, pitch) uint16} of the occupied bricks."""
    keys = m.occupied_keys()
    v = m.votes.cpu().numpy().view(np.uint16).reshape(m.capacity, B ** 3, m.pitch) if len(keys) else None
    return {tuple(k): v[s].copy() for k, s in zip(keys.tolist(), m.slots(keys))}


def assert_same_counters(a, b):
    ca, cb = counters(a), counters(b) if not isinstance(b, dict) else b
    assert list(ca) == list(cb) and len(ca) > 0
    for key in ca:
        assert np.array_equal(ca[key], cb[key]), key


def assert_same_extract(a, b):
    for min_obs, empty in ((1, False), (2, True)):
        got, want = a.extract(min_obs, empty), b.extract(min_obs, empty)
        assert len(want[1]) > 0 and all(torch.equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ split equals whole
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_split_equals_whole(monkeypatch, case):
    MergeStandIn().install(monkeypatch)
    whole, ref = build(case, range(6)), restatement(case)
    assert_map_equals_ref(whole, ref)
    for first, second in (((0, 2, 4), (1, 3, 5)), ((1, 3, 5), (0, 2, 4))):      # and with the operands swapped
        a, b = build(case, first), build(case, second)
        before = b.votes.clone()
        assert a.merge(b) is a and torch.equal(b.votes, before)               # the source is only read
        assert_same_counters(a, whole)
        assert_map_equals_ref(a, ref)
        assert_same_extract(a, whole)
    # three parts, two groupings
    parts = ((0, 3), (1, 4), (2, 5))
    left = build(case, parts[0]).merge(build(case, parts[1])).merge(build(case, parts[2]))
    right = build(case, parts[0]).merge(build(case, parts[1]).merge(build(case, parts[2])))
    for m in (left, right):
        assert_same_counters(m, whole)
        assert_map_equals_ref(m, ref)
        assert_same_extract(m, whole)


def _rows(values, pitch=12):
    rows = np.zeros((1, B ** 3, pitch), dtype=np.uint16)
    rows[0, :len(values), 3] = values
    rows[0, 4095, pitch - 5] = values[0]
    return torch.from_numpy(rows.view(np.int16))


def test_counters_saturate(monkeypatch):
    MergeStandIn().install(monkeypatch)
    m = sm.SemanticMap(12, V, GRIDS[(16, 12, 8)], (16, 12, 8))
    m.merge_rows([[0, -1, 2]], _rows([65535, 65534, 65534, 40000, 0]))
    m.merge_rows([[0, -1, 2]], _rows([0, 1, 2, 40000, 0]))
    got = m.votes.numpy().view(np.uint16).reshape(-1, B ** 3, 12)[0]
    assert got[:5, 3].tolist() == [65535, 65535, 65535, 65535, 0] and got[4095, 7] == 65535
    assert int(got.astype(np.int64).sum()) == 5 * 65535


# ------------------------------------------------------------------------------------------------ directory
def _filled(keys, value, C=5, **kw):
    m = sm.SemanticMap(C, V, (0.0, 0.0, 0.0), (16, 16, 16), **kw)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 3)
    rows = np.zeros((len(keys), B ** 3, m.pitch), dtype=np.int16)
    rows[:, :, 1] = value
    if len(keys):
        m.merge_rows(keys, torch.from_numpy(rows))
    return m


def test_directory_union_order_and_growth(monkeypatch):
    MergeStandIn().install(monkeypatch)
    ka, kb = [[0, 0, 0], [2, 0, 0], [-1, 5, 1]], [[3, 0, 0], [-4, 0, 0], [1, 1, 1]]
    # disjoint: the new bricks take slots in ascending key order whatever order they came in
    a, b = _filled(ka, 2, chunk_bricks=2), _filled(kb, 3, chunk_bricks=2)
    assert a.slots(ka).tolist() == [1, 2, 0]                                  # merge_rows admitted in ascending order too
    grown = a.grown
    a.merge(b)
    assert a.n_bricks == 6 and a.grown > grown and a.capacity >= 6
    assert a.slots([[-4, 0, 0], [1, 1, 1], [3, 0, 0]]).tolist() == [3, 4, 5]
    c = counters(a)
    assert all(int(c[tuple(k)][0, 1]) == 2 for k in ka) and all(int(c[tuple(k)][7, 1]) == 3 for k in kb)
    # overlapping and identical key sets
    a, b = _filled(ka, 2), _filled([ka[1], [9, 9, 9]], 5)
    a.merge(b)
    c = counters(a)
    assert a.n_bricks == 4 and int(c[(2, 0, 0)][0, 1]) == 7 and int(c[(0, 0, 0)][0, 1]) == 2 and int(c[(9, 9, 9)][0, 1]) == 5
    a, b = _filled(ka, 2), _filled(ka[::-1], 5)
    a.merge(b)
    assert a.n_bricks == 3 and all(int(r[0, 1]) == 7 and int(r[:, 0].max()) == 0 for r in counters(a).values())
    # an empty other changes nothing; an empty self becomes a copy with its bricks in ascending slot order
    before = a.votes.clone()
    assert a.merge(sm.SemanticMap(5, V, (0.0, 0.0, 0.0), (16, 16, 16))) is a and torch.equal(a.votes, before) and a.n_bricks == 3
    empty = sm.SemanticMap(5, V, (0.0, 0.0, 0.0), (16, 16, 16))
    empty.merge(b)
    assert empty.slots(empty.brick_keys()).tolist() == [0, 1, 2] and np.array_equal(empty.brick_keys(), b.brick_keys())
    assert_same_counters(empty, b)


def test_refusals_leave_the_map_as_it_was(monkeypatch):
    MergeStandIn().install(monkeypatch)
    a = _filled([[0, 0, 0], [1, 0, 0]], 2, max_bricks=3, chunk_bricks=2)
    with pytest.raises(ValueError, match="itself"):
        a.merge(a)
    with pytest.raises(ValueError, match="classes"):
        a.merge(_filled([[0, 0, 0]], 1, C=7))
    other = sm.SemanticMap(5, 0.4, (0.0, 0.0, 0.0), (16, 16, 16))
    with pytest.raises(ValueError, match="voxel size"):
        a.merge(other)
    rows = torch.zeros((2, B ** 3, a.pitch), dtype=torch.int16)
    with pytest.raises(ValueError, match="once"):
        a.merge_rows([[5, 5, 5], [5, 5, 5]], rows)
    with pytest.raises(ValueError, match="int16 rows"):
        a.merge_rows([[5, 5, 5]], rows)
    directory, pool = dict(a.directory), a.votes.clone()
    with pytest.raises(RuntimeError, match="max_bricks = 3"):
        a.merge(_filled([[1, 0, 0], [7, 0, 0], [8, 0, 0]], 9))
    assert a.directory == directory and torch.equal(a.votes, pool)
    # dims and vox_origin describe frames, not the lattice
    far = sm.SemanticMap(5, V, (-3.0, 1.0, 0.5), (8, 4, 2))
    far.merge_rows([[1, 0, 0]], torch.ones((1, B ** 3, far.pitch), dtype=torch.int16))
    a.merge(far)
    assert int(counters(a)[(1, 0, 0)][0, 1]) == 3 and a.n_bricks == 2


def test_occupied_keys_leave_out_the_all_zero_bricks(monkeypatch):
    MergeStandIn().install(monkeypatch)
    case = CASES[3]
    m, ref = build(case, range(6)), restatement(case)
    m.slots([[50, 50, 50]], create=True, device="cpu")                        # a brick a frame selected and never voted into
    occupied = [tuple(k) for k in m.occupied_keys().tolist()]
    assert occupied == sorted(ref.bricks()) and 0 < len(occupied) < m.n_bricks
    assert sm.SemanticMap(5, V, (0.0, 0.0, 0.0), (16, 16, 16)).occupied_keys().shape == (0, 3)
    assert [tuple(k) for k in m.occupied_keys(chunk_bricks=3).tolist()] == occupied


# ------------------------------------------------------------------------------------------------ save / load
def test_save_load_round_trip_and_resume(monkeypatch, tmp_path):
    MergeStandIn().install(monkeypatch)
    case = CASES[1]
    m, whole = build(case, (0, 1, 2)), build(case, range(6))
    m.slots([[-50, 0, 0]], create=True, device="cpu")                         # an all-zero brick, first by key
    path = m.save(str(tmp_path / "half.occmap"), chunk_bricks=3)
    n = len(m.occupied_keys())
    head = len(sm.MAP_MAGIC) + sm.MAP_HEADER.itemsize
    assert 0 < n < m.n_bricks and os.path.getsize(path) == head + n * (12 + m.brick_bytes)    # zero bricks stay out
    data = open(path, "rb").read()
    assert data[:8] == b"OCCDMAP1" and np.array_equal(np.frombuffer(data[head:head + 12 * n], "<i4").reshape(n, 3), m.occupied_keys())
    back = sm.SemanticMap.load(path, device="cpu", chunk_bricks=4)
    assert (back.n_classes, back.pitch, back.voxel_size, back.vox_origin, back.dims) == (m.n_classes, m.pitch, m.voxel_size, m.vox_origin, m.dims)
    assert back.n_bricks == n and back.slots(back.brick_keys()).tolist() == list(range(n))
    assert_same_counters(back, m)
    # load, then merge into the map of the other frames: the map of all frames
    rest = build(case, (3, 4, 5))
    rest.merge(sm.SemanticMap.load(path, device="cpu"))
    assert_same_counters(rest, whole)
    assert_map_equals_ref(rest, restatement(case))
    # an empty map round-trips too
    assert sm.SemanticMap.load(sm.SemanticMap(5, V, (0.0, 1.0, 2.0), (4, 4, 4)).save(str(tmp_path / "e.occmap")), device="cpu").n_bricks == 0
    # refusals name the file
    short, magic, edge = (str(tmp_path / name) for name in ("short.occmap", "magic.occmap", "edge.occmap"))
    open(short, "wb").write(data[:-1])
    with pytest.raises(ValueError, match=r"short\.occmap: %d bytes, its header announces %d" % (len(data) - 1, len(data))):
        sm.SemanticMap.load(short, device="cpu")
    open(magic, "wb").write(b"OCCDMAP2" + data[8:])
    with pytest.raises(ValueError, match=r"magic\.occmap is not"):
        sm.SemanticMap.load(magic, device="cpu")
    h = np.frombuffer(data[8:head], dtype=sm.MAP_HEADER).copy()
    h["brick"] = 8
    open(edge, "wb").write(data[:8] + h.tobytes() + data[head:])
    with pytest.raises(ValueError, match=r"edge\.occmap holds bricks of edge 8"):
        sm.SemanticMap.load(edge, device="cpu")
    with pytest.raises(RuntimeError, match="max_bricks"):
        sm.SemanticMap.load(path, device="cpu", max_bricks=n - 1)


# ------------------------------------------------------------------------------------------------ argument checks
def test_map_merge_entry_point_validates_arguments(hip_lib):
    buf = (ctypes.c_float * 64)()
    ptr = (ctypes.addressof(buf) + 63) & ~63             # aligned dummy address, never dereferenced: every call is rejected
    host = np.zeros((2, 2), dtype=np.int32)

    def args():
        a = hip.MapMergeArgs()
        a.votes = a.src = a.table = ptr
        a.n, a.capacity, a.src_capacity, a.pitch, a.split = 2, 4, 3, 20, 0
        return a

    merge = hip_lib.occd_map_merge
    assert merge(None, None) == -1
    for field, value in (("votes", None), ("src", None), ("table", None), ("pitch", 6), ("pitch", 36), ("pitch", 0), ("pitch", 2),
                         ("n", -1), ("capacity", 0), ("src_capacity", 0), ("votes", ptr + 8), ("src", ptr + 4), ("split", 3),
                         ("split", 16), ("split", -1)):
        a = args()
        setattr(a, field, value)
        assert merge(ctypes.byref(a), None) == -1, (field, value)
    for row in ((4, 0), (-1, 0), (0, 3), (0, -1)):                             # what the kernel would skip, the host copy refuses
        a = args()
        host[1] = row
        a.table_host = host.ctypes.data
        assert merge(ctypes.byref(a), None) == -1, row
    a = args()
    a.n = 0
    assert merge(ctypes.byref(a), None) == 0                                   # nothing to do, nothing launched
    for field in ("votes", "src", "table"):                                    # and an empty table does not excuse a null pointer
        a = args()
        a.n = 0
        setattr(a, field, None)
        assert merge(ctypes.byref(a), None) == -1, field
    assert hip.ABI_VERSION == 22 and ctypes.sizeof(hip.MapMergeArgs) == 4 * 8 + 5 * 4 + 4 and "occd_map_merge" in hip.EXPORTS


# ------------------------------------------------------------------------------------------------ two ranks over gloo
RANK_CASE = CASES[3]
SCENARIOS = (("round-robin", 256), ("rank 1 empty", 1))


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))


def _rank_frames(name, rank):
    return tuple(range(rank, 6, 2)) if name == "round-robin" else (tuple(range(6)) if rank == 0 else ())


def _ranks_worker(rank, world, port, q):
    MergeStandIn().install_in_process()
    _init(rank, world, port)
    out = []
    for name, chunk in SCENARIOS:
        m = build(RANK_CASE, _rank_frames(name, rank))
        assert sm.merge_over_ranks(m, chunk_bricks=chunk) is m
        out.append((counters(m), m.brick_keys()))
    bad = sm.SemanticMap(5 + rank, V, (0.0, 0.0, 0.0), (4, 4, 4))
    try:
        sm.merge_over_ranks(bad)
        refused = None
    except ValueError as e:
        refused = str(e)
    q.put((rank, out, refused))
    dist.barrier()
    dist.destroy_process_group()


def _run_ranks(worker, *extra):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, q) + extra) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = {}
        for _ in range(2):
            r = q.get(timeout=120)
            got[r[0]] = r[1:]
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return got


def test_two_ranks_end_with_the_map_of_all_frames(monkeypatch):
    got = _run_ranks(_ranks_worker)
    MergeStandIn().install(monkeypatch)
    want = counters(build(RANK_CASE, range(6)))
    assert len(want) > 1                                                       # chunk_bricks = 1 exchanges several chunks
    for rank in (0, 1):
        out, refused = got[rank]
        for (name, _), (have, keys) in zip(SCENARIOS, out):
            assert list(have) == list(want), (rank, name)
            assert all(np.array_equal(have[k], want[k]) for k in want), (rank, name)
            assert set(want) <= {tuple(k) for k in keys.tolist()}
        assert refused is not None and "n_classes" in refused                  # raised on every rank
    # one rank, or no process group: nothing is touched
    m = build(RANK_CASE, (0,))
    before = m.votes.clone()
    assert sm.merge_over_ranks(m) is m and torch.equal(m.votes, before)


# ------------------------------------------------------------------------------------------------ the model hook
def _hook_install_in_process():
    MergeStandIn().install_in_process()
    hip.map_sample = SampleStandIn().sample
    hip.ssc_confusion = _confusion_stand_in
    hip.argmax_labels_u16 = lambda logits, lut=None: logits.argmax(1).to(torch.int16)


def _hook_run(stub_kw, steps, out_dir, root, sub):
    """One validation epoch -> (the map's returned statistics, the mapped confusion matrix, the PLY paths, warnings)."""
    from occdepth_amd.models.OccDepth import OccDepth
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), out_dir, root, min_obs=1, frames=True,
                                        submission_dir=sub, **stub_kw)
    returned = {}

    def end(step_type):
        before = len(stub.hists)
        returned["stats"] = OccDepth._map_epoch_end(stub, step_type)
        returned["mapped"] = stub.hists[before].numpy().copy()                 # _epoch_stats saw the mapped metric first
        returned["summed"] = len(stub.hists) - before                          # 1: the map's metric did not go that way
        return returned["stats"]
    stub._map_epoch_end = end
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _epoch(stub, "val", steps)
    stats = {k: np.asarray(v).copy() for k, v in returned["stats"].items()}
    assert stub.semantic_map["maps"] == {} and stub.semantic_map["kept"] == {}
    return {"stats": stats, "mapped": returned["mapped"], "summed": returned["summed"],
            "paths": [os.path.basename(p) for p in stub.semantic_map["paths"]],
            "warned": [str(w.message) for w in caught if "more than one rank" in str(w.message)],
            "logged": {k: np.asarray(v).copy() for k, v in stub.logged_keys.items() if "map" in k}}


HOOK_DEAL = {"plain": ((0,), (1, 2)), "repeat": ((0, 1), (1, 2))}              # steps per rank; "repeat" feeds step 1 to both


def _hook_worker(rank, world, port, q, tmp):
    _hook_install_in_process()
    _init(rank, world, port)
    steps = _hook_steps()
    root = os.path.join(tmp, "sequences")
    out = {}
    for name, kw in (("plain", {}), ("repeat", {}), ("off", {"gather": False})):
        mine = [steps[i] for i in HOOK_DEAL["plain" if name == "off" else name][rank]]
        out_dir = os.path.join(tmp, "maps_" + name + ("_%d" % rank if name == "off" else ""))
        out[name] = _hook_run(kw, mine, out_dir, root, os.path.join(tmp, "sub_" + name))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _same_stats(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_model_hook_under_two_ranks(monkeypatch, tmp_path):
    root = _hook_world(tmp_path)
    got = _run_ranks(_hook_worker, str(tmp_path))
    MergeStandIn().install(monkeypatch)
    for name, fn in (("map_sample", SampleStandIn().sample), ("ssc_confusion", _confusion_stand_in),
                     ("argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))):
        monkeypatch.setattr(hip, name, fn)
    steps = _hook_steps()
    one = _hook_run({}, steps, str(tmp_path / "maps_one"), str(root), str(tmp_path / "sub_one"))
    assert one["summed"] == 2 and not one["warned"]                            # one process: both metrics go through _epoch_stats
    plys = ["val_03_gt.ply", "val_03_pred.ply", "val_08_gt.ply", "val_08_pred.ply"]
    r0, r1 = got[0][0]["plain"], got[1][0]["plain"]
    for r in (r0, r1):
        assert _same_stats(r["stats"], one["stats"]) and r["summed"] == 1 and not r["warned"]
        assert np.array_equal(r["logged"]["val_map/mIoU"], one["logged"]["val_map/mIoU"])
    assert np.array_equal(r0["mapped"] + r1["mapped"], one["mapped"]) and r0["mapped"].sum() > 0 and r1["mapped"].sum() > 0
    assert sorted(p for p in r0["paths"] if p.endswith(".ply")) == plys and not [p for p in r1["paths"] if p.endswith(".ply")]
    assert sorted(os.listdir(tmp_path / "maps_plain")) == plys
    for name in plys:                                                          # rank 0 wrote the map of all frames
        assert open(tmp_path / "maps_plain" / name, "rb").read() == open(tmp_path / "maps_one" / name, "rb").read()
    labels = lambda d: sorted(os.path.join(os.path.relpath(w, d), f) for w, _, fs in os.walk(d) for f in fs)
    assert labels(tmp_path / "sub_plain") == labels(tmp_path / "sub_one") and len(labels(tmp_path / "sub_one")) == 4
    assert sorted(p for r in (r0, r1) for p in r["paths"] if p.endswith(".label")) == sorted(p for p in one["paths"] if p.endswith(".label"))
    # a frame fed to both ranks: one warning, count 1, on every rank
    for rank in (0, 1):
        warned = got[rank][0]["repeat"]["warned"]
        assert len(warned) == 1 and warned[0].startswith("occdepth_amd: 1 frame(s)"), warned
    # gather off: every rank is a single process over its own frames
    for rank in (0, 1):
        alone = _hook_run({"gather": False}, [steps[i] for i in HOOK_DEAL["plain"][rank]], str(tmp_path / ("alone_%d" % rank)),
                          str(root), str(tmp_path / ("sub_alone_%d" % rank)))
        r = got[rank][0]["off"]
        assert _same_stats(r["stats"], alone["stats"]) and np.array_equal(r["mapped"], alone["mapped"]) and r["summed"] == 2
        assert r["paths"] == alone["paths"] and not r["warned"]
        assert sorted(os.listdir(tmp_path / ("maps_off_%d" % rank))) == sorted(os.listdir(tmp_path / ("alone_%d" % rank)))
    assert not _same_stats(got[0][0]["off"]["stats"], one["stats"])            # which is not the map of all frames


def test_save_maps_switch(monkeypatch, tmp_path):
    from occdepth_amd.models.OccDepth import OccDepth
    MergeStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    monkeypatch.setattr(hip, "argmax_labels_u16", lambda logits, lut=None: logits.argmax(1).to(torch.int16))
    root = _hook_world(tmp_path)
    stub = OccDepth.enable_semantic_map(_hook_stub(semantic_map=None), str(tmp_path / "maps"), str(root), save_maps=True)
    assert stub.semantic_map["gather"] is True and stub.semantic_map["save_maps"] is True
    steps = _hook_steps()
    _epoch(stub, "val", steps)
    names = sorted(os.listdir(tmp_path / "maps"))
    assert [n for n in names if n.endswith(".occmap")] == ["val_03_gt.occmap", "val_03_pred.occmap", "val_08_gt.occmap", "val_08_pred.occmap"]
    back = sm.SemanticMap.load(str(tmp_path / "maps" / "val_08_pred.occmap"), device="cpu")
    coords, labels, n_obs = back.extract(min_obs=1)
    verts, _ = sm.read_ply(str(tmp_path / "maps" / "val_08_pred.ply"))
    assert len(labels) > 0 and np.array_equal(verts["label"], labels.numpy()) and back.n_classes == HOOK_C


# ------------------------------------------------------------------------------------------------ the offline tool
def test_map_sequence_tool_saves_and_resumes(monkeypatch, tmp_path, capsys):
    import pickle
    tool = _tool()
    MergeStandIn().install(monkeypatch)
    monkeypatch.setattr(hip, "ssc_confusion", _confusion_stand_in)
    dims, C = (16, 12, 8), 20
    origin = GRIDS[dims]
    line = "1 0 0 %g 0 1 0 0 0 0 1 %g\n"
    seq = _write_sequence(tmp_path / "08", line % (0, 0) + line % (0, 0.4) + line % (0.2, 1.0) + line % (3.6, 0.2))
    pkl = tmp_path / "pkl"
    os.makedirs(pkl)
    for n, (lab, mask) in enumerate(frames_for(dims, C, 23, 4, masked=True)):
        with open(pkl / ("%06d.pkl" % n), "wb") as f:
            pickle.dump({"y_pred": lab.astype(np.uint16), "target": np.roll(lab, 1, axis=0).astype(np.uint16), "fov_mask_1": mask.reshape(-1)}, f)

    def run(out, *more):
        args = tool.parser().parse_args(["--poses", seq, "--pred", str(pkl), "--gt", str(pkl), "--out", str(tmp_path / out), "--fov",
                                         "--dims", "16", "12", "8", "--origin"] + [str(o) for o in origin] + list(more))
        return tool.run(args, device=torch.device("cpu"))

    whole, _ = run("whole")
    run("first", "--frame-range", "0", "1", "--save-map", str(tmp_path / "kept" / "first"))
    assert sorted(os.listdir(tmp_path / "kept")) == ["first_gt.occmap", "first_pred.occmap"]
    both, _ = run("both", "--frame-range", "2", "3", "--load-map", str(tmp_path / "kept" / "first"))
    for role in ("pred", "gt"):
        assert_same_counters(both[role], whole[role])
        data = open(tmp_path / ("both_%s.ply" % role), "rb").read()
        assert data == open(tmp_path / ("whole_%s.ply" % role), "rb").read()
        assert data != open(tmp_path / ("first_%s.ply" % role), "rb").read()
    assert "merged" in capsys.readouterr().out


def test_gather_and_save_are_switched_by_the_environment(monkeypatch, tmp_path):
    import golden_cases as gc
    from occdepth_amd.configs import PROJECT_RES
    from occdepth_amd.models.OccDepth import OccDepth

    def state():
        cfg, _ = gc.occdepth_config("kitti_flosp_small")
        return OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                        class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                        project_res=PROJECT_RES, config=cfg).semantic_map

    for var in ("OCCDEPTH_MAP_GATHER", "OCCDEPTH_MAP_SAVE", "OCCDEPTH_MAP_FRAMES", "OCCDEPTH_MAP_SUBMISSION", "OCCDEPTH_MAP_VIEWS"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("OCCDEPTH_MAP_DIR", str(tmp_path / "maps"))
    monkeypatch.setenv("OCCDEPTH_MAP_POSES", str(tmp_path / "seq"))
    st = state()
    assert (st["gather"], st["save_maps"], st["seen"]) == (True, False, {})
    monkeypatch.setenv("OCCDEPTH_MAP_GATHER", "0")
    monkeypatch.setenv("OCCDEPTH_MAP_SAVE", "1")
    st = state()
    assert (st["gather"], st["save_maps"]) == (False, True)
