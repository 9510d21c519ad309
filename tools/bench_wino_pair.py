"""K10h with one cout block per work item (cout_blocks = 1, max_workgroups = -1: today's form) against the cout-pair form
(cout_blocks = 2) on every fused-Winograd launch geometry of the config-2 frame (dev tool, GPU):

    python tools/bench_wino_pair.py > profiles/wino_cout_pair_ab.txt

N(0,1) data as in tools/bench_wino_split.py.  Each form is captured into a graph of `iters` back-to-back launches and the
graph is replayed between stream events: a warm-up replay, then three rounds; `best` and `worst` are the fastest and the
slowest round per launch, `spread` is (worst - best) / best.  The two outputs are compared with torch.equal in the same run.
`rule` is what hip.wino_cout_pair_wins says; `wins` is the convention of profiles/dwconv_stage_ab.txt: the pair form's WORST
round is faster than the one-block form's BEST round.  The per-frame sums apply the frame's launch counts to the launches that
hip.wino_f16x2_wins sends to K10h (the others run K10 in the frame and are listed for reference)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip
from bench_wino_split import GEOMETRIES


def graph_rounds(fn, iters):
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
    return min(ts), max(ts)


def main():
    hip.load()
    torch.manual_seed(0)
    print(f"{'geometry':28s} {'frame':>5s} {'one best':>9s} {'worst':>9s} {'spread':>7s} {'pair best':>9s} {'worst':>9s} {'spread':>7s} "
          f"{'one / pair':>10s}  equal  wins   rule")
    tot = {"one": 0.0, "pair": 0.0, "wins": 0.0, "rule": 0.0}
    for cin, cout, H, W, with_res, n in GEOMETRIES:
        x = torch.randn(2, cin, H, W, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.1
        sc, sh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda")
        res = torch.randn(2, cout, H, W, device="cuda") if with_res else None
        y1, y2 = torch.empty(2, cout, H, W, device="cuda"), torch.empty(2, cout, H, W, device="cuda")
        u16 = hip.wino_pack_weights_f16x2(w, sc)
        iters = max(5, min(50, int(20.0 / (1e-6 * cin * cout * H * W / 2e3 + 0.02))))

        def launch(blocks, y):
            return hip.conv2d_3x3_fused(x, u16, cout, sh, "leaky", res=res, res_first=True, out=y, max_workgroups=-1,
                                        cout_blocks=blocks)

        b1, w1 = graph_rounds(lambda: launch(1, y1), iters)
        b2, w2 = graph_rounds(lambda: launch(2, y2), iters)
        same = torch.equal(y1, y2)
        wins, rule = w2 < b1, hip.wino_cout_pair_wins(2, cin, cout, H, W)
        in_frame = hip.wino_f16x2_wins(2, cin, cout, H, W)
        if in_frame:
            tot["one"] += n * b1
            tot["pair"] += n * b2
            tot["wins"] += n * (b2 if wins else b1)
            tot["rule"] += n * (b2 if rule else b1)
        print(f"{cin:4d}>{cout:<4d} @2x{H}x{W:<10d} {'K10h' if in_frame else 'K10':>5s} {b1:9.4f} {w1:9.4f} {100 * (w1 - b1) / b1:6.1f}% "
              f"{b2:9.4f} {w2:9.4f} {100 * (w2 - b2) / b2:6.1f}% {b1 / b2:10.3f}  {str(same):5s}  {str(wins):5s}  {rule}", flush=True)
    print(f"per frame over the K10h launches (best rounds, launch counts applied): one block {tot['one']:.3f} ms, pair everywhere "
          f"{tot['pair']:.3f} ms, pair where it wins {tot['wins']:.3f} ms, by the rule {tot['rule']:.3f} ms")


if __name__ == "__main__":
    main()
