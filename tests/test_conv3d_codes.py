"""What the 3-D implicit-GEMM entry points (K2: csrc/conv3d_igemm.hip, K2b: csrc/conv3d_bf16.hip) accept, return and launch.

tests/golden/conv3d_codes.json was recorded by tools/record_conv3d_codes.py BEFORE the host halves of the two files -- validation,
the phase-consistency check, the parameter fill and the launch tail -- were merged into csrc/conv3d_tile.h.  The replay must give
the same return code for every descriptor and entry point, and on the GPU the same profile rows and output bytes per launch."""
import collections
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_conv3d_codes", os.path.join(ROOT, "tools", "record_conv3d_codes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(ROOT, "tests", "golden", "conv3d_codes.json")) as _f:
    GOLDEN = json.load(_f)


def test_return_codes(hip_lib):
    """Placeholder pointers (nothing is dereferenced on the host): this must never run where a device would receive them."""
    if torch.cuda.is_available():
        pytest.skip("the return-code table is replayed on machines without a device only")
    assert GOLDEN["calls"] == rec.CALLS
    assert set(GOLDEN["codes"]) == set(rec.BASES)
    # the table holds OCCD_EINVAL (1), OCCD_ELAUNCH (2) and OCCD_ENOMEM (3) for both kernels: it cannot pass on rejects alone
    seen = collections.defaultdict(set)
    for rows in GOLDEN["codes"].values():
        assert set(rows) == {name for name, _, _ in rec.perturbations()}
        for codes in rows.values():
            assert len(codes) == len(rec.CALLS)
            for call, c in zip(rec.CALLS, codes):
                seen[call.split("_")[0]].add(c)
    assert seen == {"k2": {"1", "2", "3"}, "k2b": {"1", "2", "3"}}
    table = rec.record_codes()
    bad = [(base, name, [(c, w, g) for c, w, g in zip(rec.CALLS, want, table[base][name]) if w != g])
           for base, rows in GOLDEN["codes"].items() for name, want in rows.items() if table[base][name] != want]
    assert not bad, f"{len(bad)} descriptors return other codes than recorded (call, recorded, now); the first: {bad[0]}"


@pytest.mark.gpu
def test_launch_rows_and_output_hashes(hip_lib):
    assert set(GOLDEN["launches"]) == set(rec.launches())
    table = rec.record_launches()
    bad = [(name, want, table[name]) for name, want in GOLDEN["launches"].items() if table[name] != want]
    assert not bad, f"{len(bad)} launches differ from the recorded table (name, recorded, now); the first: {bad[0]}"
