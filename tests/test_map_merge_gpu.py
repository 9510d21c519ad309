"""GPU: occd_map_merge (K33) against its numpy restatement min(dst + src, 65535), SemanticMap.merge / merge_rows against
the map of all frames and `MapRef`, save and load on the GPU, and merge_over_ranks between two processes that share the
GPU.  Counters are integers: every comparison is exact equality.  The shapes are those of tests/test_map_gpu.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from occdepth_amd import hip
from occdepth_amd import semantic_map as sm
from test_map import B, GRIDS, V, assert_map_equals_ref, frames_for, pose, sequence
from test_map_gpu import CASES, IDS, _tensor, built
from test_shard_gloo import _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(case, which):
    dims, C, label_bytes, masked = case
    frames, poses = frames_for(dims, C, 100 * C + label_bytes, 6, label_bytes, masked), sequence(dims)
    m = sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=8)
    for i in which:
        lab, mask = frames[i]
        m.integrate(_tensor(lab), poses[i], mask=None if mask is None else torch.from_numpy(mask).cuda())
    return m


@functools.lru_cache(maxsize=None)
def halves(case):
    """(frames 0 2 4, frames 1 3 5), shared by the tests and never changed: a test merges into a clone or a fresh map."""
    return build(case, (0, 2, 4)), build(case, (1, 3, 5))


def u16(t):
    return t.cpu().numpy().view(np.uint16).astype(np.int64)


def restate(dst, src, table):
    out = u16(dst)
    s = u16(src)
    for slot, row in table:
        out[slot] = np.minimum(out[slot] + s[row], 65535)
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_equals_the_restatement(case):
    a, b = halves(case)
    rng = np.random.default_rng(5)
    n = min(a.n_bricks, b.n_bricks) - 2                                    # some bricks of the pool stay out of the table
    table = np.stack([rng.permutation(a.n_bricks)[:n], rng.permutation(b.n_bricks)[:n]], 1).astype(np.int32)
    assert n > 2
    for split in (0, 1, 2, 4, 8):
        votes = a.pool().clone()
        dev_table, host_table = a.upload(table, votes.device)
        hip.map_merge(votes, b.pool(), dev_table, table_host=host_table, split=split)
        want = restate(a.pool(), b.pool(), table)
        got = u16(votes)
        assert np.array_equal(got, want), split                            # the table's bricks, and every other byte as before
        untouched = np.setdiff1d(np.arange(a.capacity), table[:, 0])
        assert len(untouched) and np.array_equal(got[untouched], u16(a.pool())[untouched])
        assert (got != u16(a.pool())).any()


def test_bad_table_rows_are_skipped():
    a, b = halves(CASES[3])
    votes = a.pool().clone()
    table = np.array([[-1, 0], [a.capacity, 1], [0, b.capacity], [1, -1], [2, 3], [-(1 << 31), (1 << 31) - 1]], dtype=np.int32)
    hip.map_merge(votes, b.pool(), torch.from_numpy(table).cuda())         # without the host copy, which would refuse them
    want = restate(a.pool(), b.pool(), [(2, 3)])
    assert np.array_equal(u16(votes), want) and (want[2] != u16(a.pool())[2]).any()
    with pytest.raises(RuntimeError, match="occd_map_merge"):
        hip.map_merge(votes, b.pool(), torch.from_numpy(table).cuda(), table_host=torch.from_numpy(table))
    assert hip.map_merge(votes, b.pool(), torch.zeros((0, 2), dtype=torch.int32, device="cuda")) is votes
    assert np.array_equal(u16(votes), want)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_split_equals_whole(case):
    dims, C, label_bytes, masked = case
    whole, ref = built(*case)
    a, b = halves(case)
    m = sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=8).merge(a).merge(b)
    assert_map_equals_ref(m, ref)
    for min_obs, empty in ((1, False), (2, True)):
        assert all(torch.equal(g, w) for g, w in zip(m.extract(min_obs, empty), whole.extract(min_obs, empty)))
    frames = frames_for(dims, C, 100 * C + label_bytes, 6, label_bytes, masked)
    for (lab, mask), P in zip(frames, sequence(dims)):
        kw = dict(own=_tensor(lab), own_mask=None if mask is None else torch.from_numpy(mask).cuda(), exclude_self=False, keep_own=True)
        got, want = m.sample(P, **kw), whole.sample(P, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int((want[1] != 0).sum()) > 0


def test_counters_saturate_and_padding_stays_zero():
    m = sm.SemanticMap(5, V, (0.0, 0.0, 0.0), (16, 16, 16))               # pitch 8: three padding counters per row
    lab = np.full((16, 16, 16), 3, dtype=np.uint8)
    m.integrate(_tensor(lab), pose())
    slot = int(m.slots([[0, 0, 0]])[0])
    rows = np.zeros((2, B ** 3, 8), dtype=np.uint16)
    first, second = [65535, 65534, 65534, 40000, 0], [0, 1, 2, 40000, 0]
    rows[0, :5, 1], rows[1, :5, 1] = first, second
    for r in rows:
        m.merge_rows([[0, 0, 0]], torch.from_numpy(r[None].view(np.int16)))     # from the host
    got = u16(m.pool())[slot]
    assert got[:5, 1].tolist() == [65535, 65535, 65535, 65535, 0] and (got[:, 3] == 1).all()
    assert not got[:, 5:].any() and int(got.sum()) == 4 * 65535 + 4096


def test_host_rows_pool_rows_torch_and_reruns_give_the_same_bytes():
    case = CASES[1]
    a, b = halves(case)
    dims, C = case[0], case[1]
    fresh = lambda: sm.SemanticMap(C, V, GRIDS[dims], dims, chunk_bricks=8).merge(a)
    direct = fresh().merge(b)                                              # straight from b.pool()
    again = fresh().merge(b)
    keys = b.brick_keys()
    rows = b.pool()[torch.from_numpy(b.slots(keys).astype(np.int64)).cuda()]
    via_host = fresh().merge_rows(keys, rows.cpu())
    via_device = fresh().merge_rows(keys[::-1].copy(), rows.flip(0).contiguous())
    assert np.array_equal(direct.brick_keys(), via_host.brick_keys())
    for other in (again, via_host, via_device):
        assert other.directory == direct.directory and torch.equal(other.votes, direct.votes)
    # the torch-operator formulation: int32 add, clamp, index
    base = fresh()
    slots = torch.from_numpy(base.slots(keys, create=True, device="cuda").astype(np.int64)).cuda()
    pool = base.pool()
    total = (pool[slots].to(torch.int32) & 0xFFFF) + (rows.to(torch.int32) & 0xFFFF)
    pool[slots] = total.clamp(max=65535).to(torch.int16)
    assert base.directory == direct.directory and torch.equal(base.votes, direct.votes)


def test_save_and_load_on_the_gpu(tmp_path):
    whole, ref = built(*CASES[0])
    path = whole.save(str(tmp_path / "whole.occmap"), chunk_bricks=5)
    back = sm.SemanticMap.load(path, chunk_bricks=7)
    assert back.votes.is_cuda and back.n_bricks == len(whole.occupied_keys()) == len(ref.bricks())
    assert_map_equals_ref(back, ref)
    assert all(torch.equal(g, w) for g, w in zip(back.extract(), whole.extract()))
    a, b = halves(CASES[0])
    resumed = sm.SemanticMap.load(a.save(str(tmp_path / "a.occmap"))).merge(b)
    assert_map_equals_ref(resumed, ref)


def test_two_ranks_on_one_gpu():
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "map_ranks_worker.py")], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=150)
            outs.append((p.returncode, out))
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        raise AssertionError("map rank workers timed out:\n" + "\n".join(o for _, o in outs))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rank, (rc, out) in enumerate(outs):
        line = [l for l in out.splitlines() if l.startswith("MAP_RANKS_RESULT ")]
        assert rc == 0 and line, out[-3000:]
        r = json.loads(line[-1][len("MAP_RANKS_RESULT "):])
        assert r["rank"] == rank and r["world"] == 2 and r["bricks"] > 4
        assert r["round_robin"] and r["rank0_only"] and r["round_robin_device"] == r["rank0_only_device"] == "cuda", r
