"""One rank of tests/test_map_merge_gpu.py::test_two_ranks_on_one_gpu: RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in
the environment, gloo between the processes, the maps on the GPU they share.  Frames are dealt round-robin, then all to
rank 0; after semantic_map.merge_over_ranks every rank must hold the counters of the map of all frames, which it builds
for itself.  Steps run in order and the first failure ends the process: nothing further is started.  The last line is
`MAP_RANKS_RESULT <json>`."""
import datetime
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from occdepth_amd import semantic_map as sm  # noqa: E402
from test_map import GRIDS, V, frames_for, sequence  # noqa: E402

DIMS, C, LABEL_BYTES, MASKED = (16, 12, 8), 12, 1, True


def build(which):
    frames, poses = frames_for(DIMS, C, 100 * C + LABEL_BYTES, 6, LABEL_BYTES, MASKED), sequence(DIMS)
    m = sm.SemanticMap(C, V, GRIDS[DIMS], DIMS, chunk_bricks=8)
    for i in which:
        lab, mask = frames[i]
        m.integrate(torch.from_numpy(lab).cuda(), poses[i], mask=torch.from_numpy(mask).cuda())
    return m


def occupied(m):
    keys = m.occupied_keys()
    slots = torch.from_numpy(m.slots(keys).astype(np.int64)).to(m.votes.device)
    return keys, m.pool().index_select(0, slots)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    want_keys, want_rows = occupied(build(range(6)))
    result = {"rank": rank, "world": world, "bricks": len(want_keys)}
    for name, which, chunk in (("round_robin", tuple(range(rank, 6, world)), 4), ("rank0_only", tuple(range(6)) if rank == 0 else (), 256)):
        m = build(which)
        sm.merge_over_ranks(m, chunk_bricks=chunk)
        keys, rows = occupied(m)
        result[name] = bool(np.array_equal(keys, want_keys)) and bool(torch.equal(rows, want_rows))
        result[name + "_device"] = str(m.votes.device.type)
        if not result[name]:
            break
    torch.cuda.synchronize()
    print("MAP_RANKS_RESULT " + json.dumps(result), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
