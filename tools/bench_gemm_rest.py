"""The 2-D GEMMs that still split float32 operands on the fly (gemm_x3_kernel<..., PRE = 0>) against the same work on the f16x2
weight image (dev tool, GPU):

    python tools/bench_gemm_rest.py >> profiles/gemm_f16x2_rest_ab.txt

  * the two Winograd-domain products of the config-2 frame with their transforms: the present form (wino_input -> K16 on
    float32 V . U -> wino_output) against the channel-major one (hip.WinoCM: wino_input_cm -> K16 on the image of U^T ->
    wino_output_cm), whole convolution and piece by piece;
  * the weight-on-the-left launches below 256 rows (project convolutions with gate and skip, the 192-row expand): float32
    operands against the image with tile_hint 0 and the forced tile variants 1 .. 5.

N(0,1) data.  Every timing is a replayed graph of `iters` back-to-back launches: warm-up replay, then the best of three replays
between stream events; `spread` is (worst - best) / best.  A geometry whose gain lies inside the larger of the two spreads is
"no gain"."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

# (B, Cin, Cout, H, W): the two UpSampleBN second convolutions that take the unfused Winograd path
WINO = [(2, 1280, 1280, 24, 77), (2, 640, 640, 47, 153)]
# (M, N, K, launches per frame, gate + skip?, act) at batch 2: the PRE = 0 rows of profiles/r06_frame_per_launch.txt
REST = [(48, 28365, 288, 6, True, None), (80, 7191, 480, 6, True, None), (192, 112850, 32, 1, False, "swish"),
        (48, 28365, 192, 1, False, None), (80, 7191, 288, 1, False, None), (160, 1848, 480, 1, False, None)]


def rounds(fn, iters):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    del graph
    return min(ts), (max(ts) - min(ts)) / min(ts)


def verdict(old, new):
    (t0, s0), (t1, s1) = old, new
    gain = (t0 - t1) / t0
    return "WINS" if gain > max(s0, s1) else "no gain" if abs(gain) <= max(s0, s1) else "SLOWER"


def fmt(r):
    return f"{r[0]:8.4f} ms {100 * r[1]:5.1f}%"


def wino(dev):
    print("Winograd-domain products: present form against channel-major form (ms per launch, spread)")
    for B, cin, cout, H, W in WINO:
        x = torch.randn(B, cin, H, W, device=dev)
        w = torch.randn(cout, cin, 3, 3, device=dev) / (3.0 * cin ** 0.5)
        sc, sh = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
        U = hip.winograd_weights(w)
        ucm = hip.WinoCM(w, lambda: U)
        name = f"{cin}>{cout} @{B}x{H}x{W}"
        V, Vt = hip.wino_input_transform(x), hip.wino_input_transform_cm(x)
        M = hip.matmul(V, U)
        Mt = torch.empty((16, cout, Vt.stride(1)), device=dev)[..., :Vt.shape[2]]
        hip.gemm_x3(ucm.image, Vt, out=Mt)
        T, flops = Vt.shape[2], 2.0 * 16 * Vt.shape[2] * cin * cout
        rows = [("input transform", lambda: hip.wino_input_transform(x), lambda: hip.wino_input_transform_cm(x)),
                ("product", lambda: hip.matmul(V, U), lambda: hip.gemm_x3(ucm.image, Vt, out=Mt)),
                ("output transform", lambda: hip.wino_output_transform(M, (B, cout, H, W), sc, sh, "leaky"),
                 lambda: hip.wino_output_transform_cm(Mt, (B, cout, H, W), sc, sh, "leaky")),
                ("whole convolution", lambda: hip.conv2d_3x3_winograd(x, ucm, sc, sh, "leaky", cm=False),
                 lambda: hip.conv2d_3x3_winograd(x, ucm, sc, sh, "leaky", cm=True))]
        for what, old, new in rows:
            r0, r1 = rounds(old, 20), rounds(new, 20)
            extra = f"  {flops / r0[0] / 1e9:6.1f} -> {flops / r1[0] / 1e9:6.1f} TF/s" if what == "product" else ""
            print(f"  {name:24s} T={T:5d} {what:18s} present {fmt(r0)} | channel-major {fmt(r1)} | x{r0[0] / r1[0]:5.2f} "
                  f"{verdict(r0, r1)}{extra}", flush=True)
        for hint in (1, 2, 3, 4):                                # the product under the forced tile variants
            r = rounds(lambda: hip.gemm_x3(ucm.image, Vt, out=Mt, tile_hint=hint), 20)
            print(f"  {name:24s} product on the image, tile_hint {hint}: {fmt(r)}  {flops / r[0] / 1e9:6.1f} TF/s", flush=True)
        del x, w, U, ucm, V, Vt, M, Mt


def rest(dev):
    print("weight-on-the-left launches below 256 rows: float32 operands (today) against the f16x2 image (ms per launch, spread)")
    batch, tot = 2, [0.0, 0.0]
    for M, N, K, n, gated, act in REST:
        w = torch.randn(M, K, device=dev) / K ** 0.5
        b = torch.randn(batch, K, N, device=dev)
        bias = torch.randn(M, device=dev)
        kw = dict(bias=bias, act=act)
        if gated:
            kw.update(k_scale=torch.rand(batch, K, device=dev), res=torch.randn(batch, M, N, device=dev))
        out = torch.empty(batch, M, N, device=dev)
        ph = hip.GemmPacked(w, "a", split="f16x2")
        r0 = rounds(lambda: hip.gemm_x3(w, b, out=out, **kw), 50)
        name = f"{M}x{N}x{K} b{batch}{' gate+skip' if gated else ''}"
        best = None
        for hint in (0, 1, 2, 3, 4, 5):
            r = rounds(lambda: hip.gemm_x3(ph, b, out=out, tile_hint=hint, **kw), 50)
            print(f"  {name:34s} n={n} today {fmt(r0)} | image hint {hint} {fmt(r)} | x{r0[0] / r[0]:5.2f} {verdict(r0, r)}",
                  flush=True)
            if hint == 0:
                tot[0] += n * r0[0]
                tot[1] += n * r[0]
            if best is None or r[0] < best[1][0]:
                best = (hint, r)
        print(f"  {name:34s} best variant on the image: hint {best[0]} at {best[1][0]:.4f} ms")
        del w, b, out, ph, kw
    print(f"  per frame (launch counts applied, hint 0): today {tot[0]:.3f} ms, image {tot[1]:.3f} ms, "
          f"difference {tot[0] - tot[1]:.3f} ms")


def main():
    hip.load()
    torch.manual_seed(0)
    wino("cuda")
    rest("cuda")


if __name__ == "__main__":
    main()
