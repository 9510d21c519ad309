"""K10, K10h with one workgroup per item (max_workgroups = -1) and the persistent K10h (max_workgroups = 0) on every
fused-Winograd launch geometry of the config-2 frame (dev tool, GPU):

    python tools/bench_wino_persist.py > profiles/wino_persist_ab.txt

The protocol of tools/bench_wino_split.py: N(0,1) data, warm-up launches, then the best of three rounds of back-to-back
launches between stream events; `spread` is (worst - best) / best of the three rounds.  The persistent output is compared
with the form -1 bit for bit before anything is timed.  On a tree without the persistent form (conv2d_3x3_fused has no
max_workgroups) only K10 and K10h are timed, which is how the rows of the parent commit are taken."""
import inspect
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip
from bench_wino_split import GEOMETRIES, rounds

HAS_EX = "max_workgroups" in inspect.signature(hip.conv2d_3x3_fused).parameters


def main():
    hip.load()
    torch.manual_seed(0)
    print(f"{'geometry':28s} {'items':>6s} {'K10 ms':>9s} {'spread':>7s} {'K10h -1':>9s} {'spread':>7s} {'K10h 0':>9s} {'spread':>7s} "
          f"{'-1 / 0':>7s}  equal")
    tot = [0.0, 0.0, 0.0]
    for cin, cout, H, W, with_res, n in GEOMETRIES:
        x = torch.randn(2, cin, H, W, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.1
        sc, sh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda")
        res = torch.randn(2, cout, H, W, device="cuda") if with_res else None
        y = torch.empty(2, cout, H, W, device="cuda")
        u32, u16 = hip.wino_pack_weights(w, sc), hip.wino_pack_weights_f16x2(w, sc)
        iters = max(5, min(50, int(20.0 / (1e-6 * cin * cout * H * W / 2e3 + 0.02))))

        def launch(u, **kw):
            return hip.conv2d_3x3_fused(x, u, cout, sh, "leaky", res=res, res_first=True, out=y, **kw)

        t32, s32 = rounds(lambda: launch(u32), iters)
        if HAS_EX:
            same = torch.equal(launch(u16, max_workgroups=-1).clone(), launch(u16, max_workgroups=0))
            tm, sm = rounds(lambda: launch(u16, max_workgroups=-1), iters)
            tp, sp = rounds(lambda: launch(u16, max_workgroups=0), iters)
        else:
            same = None
            tm, sm = rounds(lambda: launch(u16), iters)
            tp, sp = float("nan"), float("nan")
        items = 2 * ((cout + 31) // 32) * ((((H + 1) // 2) * ((W + 1) // 2) + 127) // 128)
        for i, t in enumerate((t32, tm, tp)):
            tot[i] += n * t
        print(f"{cin:4d}>{cout:<4d} @2x{H}x{W:<10d} {items:6d} {t32:9.4f} {100 * s32:6.1f}% {tm:9.4f} {100 * sm:6.1f}% {tp:9.4f} "
              f"{100 * sp:6.1f}% {tm / tp:7.3f}  {same}", flush=True)
    print(f"per frame (launch counts applied): K10 {tot[0]:.3f} ms, K10h -1 {tot[1]:.3f} ms, K10h persistent {tot[2]:.3f} ms")


if __name__ == "__main__":
    main()
