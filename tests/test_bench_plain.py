"""The plain benchmark run (`bench.py --gpus 1 --steps K --warmup W`): the headline alone, and `--dump-outputs DIR` -- what the
last timed step returned, as DIR/<name>.npy in float32 / float64, at most 64 MB in all, the same inputs in every run.
The CPU tests pin the dump rule; the GPU test runs the command itself twice and compares the two dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
LIMIT = 64 << 20


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_budget_dtypes_and_seeded_sample(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(3)
    arrays = {"ssc_logit": torch.randn(1, 20, 256, 128, 32, generator=g),        # 21 M elements (84 MB): sampled
              "occ_logit": torch.randn(1, 2, 128, 128, 32, generator=g),          # 1 M: whole
              "depth": torch.randn(3, 5, generator=g).double(),                   # float64 stays float64
              "mask": torch.rand(4, 4, generator=g) > 0.5}                        # bool -> float32
    w1 = bench.dump_outputs(arrays, str(tmp_path / "a"))
    w2 = bench.dump_outputs({k: v.clone() for k, v in reversed(list(arrays.items()))}, str(tmp_path / "b"))
    assert w1 == w2
    files = sorted((tmp_path / "a").glob("*.npy"))
    assert sorted(f.stem for f in files) == sorted(arrays)
    assert sum(f.stat().st_size for f in files) <= LIMIT
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32)
        assert np.array_equal(a, b)                                               # the same sample in both runs
        if w1[name][0] == t.numel():
            assert a.shape == tuple(t.shape) and np.array_equal(a, t.to(torch.float64 if a.dtype == np.float64 else torch.float32).numpy())
        else:
            n = t.numel()
            idx = np.sort(np.random.default_rng([bench.DUMP_SAMPLE_SEED, n]).choice(n, a.size, replace=False))
            assert a.ndim == 1 and a.size == w1[name][0] > 0
            assert np.array_equal(a, t.reshape(-1).numpy()[idx])                  # the seeded sample of the array's elements
    assert w1["ssc_logit"][0] < arrays["ssc_logit"].numel() and w1["occ_logit"][0] == arrays["occ_logit"].numel()


def test_dump_outputs_stays_within_a_small_budget(tmp_path):
    bench = _bench()
    arrays = {f"x{i}": torch.arange(1000 * (i + 1), dtype=torch.float32) for i in range(4)}
    w = bench.dump_outputs(arrays, str(tmp_path), budget_bytes=4 * 3000)
    assert sum(n for n, _ in w.values()) <= 3000
    for name, (n, total) in w.items():
        a = np.load(tmp_path / f"{name}.npy")
        assert a.size == n and np.all(np.diff(a) > 0)                            # sorted indices of an increasing array


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    from occdepth_amd import fused
    bench = _bench()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
        t = json.loads(lines[0])
        assert t["steps"] == 3 and t["warmup"] == 2 and t["n_gpus"] == 1
        assert t["unit"] == "frames/s" and t["higher_is_better"] is True
        assert t["value"] > 0 and abs(t["value"] - 1e3 / t["ms_per_step"]) < 1e-6 * t["value"]
        assert t["dtype"] == (bench.HEAD_X3_DTYPE if fused.BF16X3 else "f32")
        assert t["config"]["graph_all"] is True and "graph_all_error" not in t["config"]
        for k in ("roofline", "stages_ms", "parity_rel_err", "extras"):          # --full only
            assert k not in t, k
        assert t["cpu_baseline"] is None
        files = sorted(d.glob("*.npy"))
        assert {"ssc_logit", "occ_logit"} <= {f.stem for f in files}
        assert sum(f.stat().st_size for f in files) <= LIMIT
        arrays = {f.stem: np.load(f) for f in files}
        for name, a in arrays.items():
            assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), name
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    for name, a in dumps[0].items():
        b = dumps[1][name]
        assert a.shape == b.shape
        assert np.abs(a - b).max() <= 1e-5 * max(float(np.abs(a).max()), 1e-30), name
