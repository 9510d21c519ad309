"""K38 on the GPU: occd_sort_pairs_u32 against numpy.argsort(kind="stable"), exactly -- keys and values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEY_SETS = ("uniform", "equal", "two", "top_digit", "low_digit", "sorted", "reverse")
BIT_RANGES = ((0, 32), (0, 31))


def shapes():
    from occdepth_amd import hip
    T = hip.SORT_TILE
    return [(1, 1), (1, 63), (1, 64), (1, 65), (3, T - 1), (3, T), (3, T + 1), (2, 3 * T + 17), (20, 100003)]


def make_keys(kind, S, n, rng):
    if kind == "uniform":
        k = rng.integers(0, 1 << 32, (S, n), dtype=np.uint64)
    elif kind == "equal":
        k = np.full((S, n), 0x9E3779B9, np.uint64)
    elif kind == "two":
        k = np.where(rng.random((S, n)) < 0.5, 0x12345678, 0x62345679).astype(np.uint64)
    elif kind == "top_digit":
        k = (rng.integers(0, 256, (S, n), dtype=np.uint64) << np.uint64(24)) | np.uint64(0x00ABCDEF)
    elif kind == "low_digit":
        k = rng.integers(0, 256, (S, n), dtype=np.uint64) | np.uint64(0x5BCDEF00)
    else:
        k = np.sort(rng.integers(0, 1 << 32, (S, n), dtype=np.uint64), axis=1)
        if kind == "reverse":
            k = k[:, ::-1]
    return np.ascontiguousarray(k).astype(np.uint32)


def reference(keys, vals, begin_bit, end_bit):
    mask = np.uint32(((1 << (end_bit - begin_bit)) - 1) << begin_bit)
    order = np.argsort(keys & mask, axis=1, kind="stable")
    return np.take_along_axis(keys, order, 1), np.take_along_axis(vals, order, 1)


def to_gpu(a):
    return torch.from_numpy(a.view(np.int32)).cuda()


def to_np(t):
    return t.cpu().numpy().view(np.uint32)


def segment_values(S, n):
    """Distinct value ranges per segment: a pair that crossed a segment boundary shows in its value."""
    return (np.arange(S, dtype=np.uint32)[:, None] * np.uint32(1 << 24) + np.arange(n, dtype=np.uint32)[None]).astype(np.uint32)


@pytest.mark.parametrize("bits", BIT_RANGES)
@pytest.mark.parametrize("shape", range(9))
def test_sorted_pairs_equal_the_stable_argsort(shape, bits, hip_lib):
    from occdepth_amd import hip
    S, n = shapes()[shape]
    rng = np.random.default_rng(17 * shape + bits[1])
    vals = segment_values(S, n)
    scratch = hip.sort_scratch(S, n, "cuda")
    for kind in KEY_SETS:
        keys = make_keys(kind, S, n, rng)
        want_k, want_v = reference(keys, vals, *bits)
        got_k, got_v = hip.sort_pairs(to_gpu(keys), to_gpu(vals), bits[0], bits[1], scratch)
        got_k, got_v = to_np(got_k), to_np(got_v)
        assert np.array_equal(got_k, want_k), (kind, S, n)
        assert np.array_equal(got_v, want_v), (kind, S, n)
        assert (got_v >> 24 == np.arange(S, dtype=np.uint32)[:, None]).all()            # no pair left its segment


def test_partial_bit_ranges_and_odd_pass_counts(hip_lib):
    """A range that does not start at bit 0, and pass counts 1, 2, 3: the result lands in either buffer."""
    from occdepth_amd import hip
    S, n = 2, hip.SORT_TILE + 5
    rng = np.random.default_rng(3)
    keys, vals = make_keys("uniform", S, n, rng), segment_values(S, n)
    for bits in ((0, 8), (4, 16), (8, 31), (5, 6), (0, 30)):
        want_k, want_v = reference(keys, vals, *bits)
        got_k, got_v = hip.sort_pairs(to_gpu(keys), to_gpu(vals), *bits)
        assert np.array_equal(to_np(got_k), want_k) and np.array_equal(to_np(got_v), want_v), bits


def test_two_calls_give_identical_bytes(hip_lib):
    from occdepth_amd import hip
    S, n = 3, 3 * hip.SORT_TILE + 17
    keys = make_keys("two", S, n, np.random.default_rng(5))
    vals = segment_values(S, n)
    runs = [hip.sort_pairs(to_gpu(keys), to_gpu(vals)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_captured_sort_replays_equal_to_eager(hip_lib):
    from occdepth_amd import hip
    S, n = 2, 3 * hip.SORT_TILE + 17
    vals = segment_values(S, n)
    inputs = [make_keys("uniform", S, n, np.random.default_rng(40 + i)) for i in range(3)]
    eager = [tuple(t.clone() for t in hip.sort_pairs(to_gpu(k), to_gpu(vals), 0, 31)) for k in inputs]
    s_keys, s_vals = to_gpu(inputs[0]), to_gpu(vals)
    w_keys, w_vals = torch.empty_like(s_keys), torch.empty_like(s_vals)              # the sort overwrites its input
    scratch = hip.sort_scratch(S, n, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.sort_pairs(w_keys.copy_(s_keys), w_vals.copy_(s_vals), 0, 31, scratch)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_k, out_v = hip.sort_pairs(w_keys.copy_(s_keys), w_vals.copy_(s_vals), 0, 31, scratch)
    for i in (1, 2, 0):
        s_keys.copy_(to_gpu(inputs[i]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_k, eager[i][0]) and torch.equal(out_v, eager[i][1]), i
