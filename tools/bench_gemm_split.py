"""The three-term bf16 weight image against the two-term fp16 one (hip.GemmPacked(w, "a", split="f16x2"), SPLIT = 2 of
csrc/gemm_x3.hip) on every GEMM of the config-2 frame that reads pre-split weights -- K16p, K21 and K16 on the A image (dev
tool, GPU):

    python tools/bench_gemm_split.py > profiles/gemm_f16x2_ab.txt

N(0,1) data; warm-up launches, then the best of three rounds of back-to-back launches between stream events (the protocol of
tools/bench_k2b_split.py).  `spread` is (worst - best) / best of the three rounds; a geometry whose gain lies inside the
larger of its two spreads is reported as "no gain"."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip
from bench_k2b_split import report, rounds

# (M, N, K, launches per frame) at batch 2: the gemm_f32x3_panel / _preA / _splitk rows of profiles/r06_frame_per_launch.txt
PANEL = [(720, 112850, 160, 1), (1440, 28365, 320, 1), (2304, 468, 384, 13), (1344, 1848, 224, 10), (288, 28365, 48, 7),
         (960, 1848, 160, 10), (480, 7191, 80, 7), (3840, 468, 640, 3), (2560, 574, 640, 1)]
PREA = [(11520, 574, 2560, 1), (2880, 7191, 640, 1), (5760, 1848, 1280, 1)]
SPLITK = [(384, 468, 2304, 12), (224, 1848, 1344, 9), (160, 1848, 960, 9), (640, 468, 3840, 3), (640, 468, 2304, 1),
          (224, 1848, 960, 1), (384, 468, 1344, 1)]


def main():
    hip.load()
    torch.manual_seed(0)
    dev, batch = "cuda", 2
    print(f"{'launch':44s} {'n':>2s} {'bf16x3 ms':>9s} {'spread':>7s} {'f16x2 ms':>9s} {'spread':>7s} {'x3/f16x2':>9s}  verdict")
    grand = [0.0, 0.0]
    for family, shapes in (("panel", PANEL), ("preA", PREA), ("splitk", SPLITK)):
        tot = [0.0, 0.0]
        for M, N, K, n in shapes:
            w = torch.randn(M, K, device=dev) / K ** 0.5
            b = torch.randn(batch, K, N, device=dev)
            bias = torch.randn(M, device=dev)
            out = hip.padded_rows((batch, M, N), dev)
            p3, ph = hip.GemmPacked(w, "a"), hip.GemmPacked(w, "a", split="f16x2")
            if family == "splitk":
                gate, res = torch.rand(batch, K, device=dev), torch.randn(batch, M, N, device=dev)
                run = lambda pa: hip.gemm_x3_splitk(pa, b, bias=bias, k_scale=gate, res=res)
            else:
                route = hip.gemm_route(M, N, K, batch, a=hip.GemmWeights(w, "a"))
                assert route.a == "bf16x3" and (route.kernel[0] == "panel") == (family == "panel")
                run = lambda pa: hip.gemm_x3(pa, b, bias=bias, act="swish", out=out)
            iters = 20 if M * N * K > 1 << 32 else 100
            r3 = rounds(lambda: run(p3), iters)
            rh = rounds(lambda: run(ph), iters)
            report(f"{family} {M}x{N}x{K} b{batch}", n, r3, rh, tot)
            del w, b, out, p3, ph
        print(f"{family} per frame (launch counts applied): bf16x3 {tot[0]:.3f} ms, f16x2 {tot[1]:.3f} ms, "
              f"difference {tot[0] - tot[1]:.3f} ms", flush=True)
        grand[0] += tot[0]
        grand[1] += tot[1]
    print(f"all three routes per frame: bf16x3 {grand[0]:.3f} ms, f16x2 {grand[1]:.3f} ms, difference {grand[0] - grand[1]:.3f} ms")


if __name__ == "__main__":
    main()
