"""K2b's three-term bf16 split against K2bh (the two-term fp16 split, SPLIT = 2 of csrc/conv3d_bf16.hip) on the ten launches
of the config-2 frame that take them (dev tool, GPU):

    python tools/bench_k2b_split.py > profiles/k2b_f16x2_ab.txt

N(0,1) data; warm-up launches, then the best of three rounds of back-to-back launches between stream events (the protocol of
tools/bench_wino_split.py).  `spread` is (worst - best) / best of the three rounds; a geometry whose gain lies inside the
larger of its two spreads is reported as "no gain"."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

# (cin, cout, dims, stride, dilation, launches per frame): the conv3d_bf16x3 rows of profiles/r06_frame_per_launch.txt
SMALL = [(256, 256, (32, 32, 4), 1, 1, 2), (256, 256, (32, 32, 4), 1, 2, 2), (256, 256, (32, 32, 4), 1, 3, 2),
         (256, 512, (32, 32, 4), 2, 1, 1)]
# (cin, cout, input dims, launches per frame): the merged phase launches of the three Upsample blocks
PHASES = [(64, 32, (128, 128, 16), 1), (128, 64, (64, 64, 8), 1), (256, 128, (32, 32, 4), 1)]


def rounds(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return min(ts), (max(ts) - min(ts)) / min(ts)


def report(label, n, r3, rh, tot):
    (t3, s3), (th, sh) = r3, rh
    gain = (t3 - th) / t3
    verdict = "f16x2" if gain > max(s3, sh) else "no gain" if abs(gain) <= max(s3, sh) else "SLOWER"
    tot[0] += n * t3
    tot[1] += n * th
    print(f"{label:44s} {n:2d} {t3:9.4f} {100 * s3:6.1f}% {th:9.4f} {100 * sh:6.1f}% {t3 / th:9.2f}  {verdict}", flush=True)


def main():
    hip.load()
    torch.manual_seed(0)
    dev = "cuda"
    print(f"{'launch':44s} {'n':>2s} {'bf16x3 ms':>9s} {'spread':>7s} {'f16x2 ms':>9s} {'spread':>7s} {'x3/f16x2':>9s}  verdict")
    tot = [0.0, 0.0]
    for cin, cout, dims, s, d, n in SMALL:
        x = hip.Vox.from_ncdhw(torch.randn(1, cin, *dims, device=dev))
        w = torch.randn(cout, cin, 3, 3, 3, device=dev) / (cin * 27) ** 0.5
        bias = torch.randn(cout, device=dev)
        odims = tuple((m + 2 * d - 2 * d - 1) // s + 1 for m in dims)
        out = hip.Vox.empty(1, odims, cout, dev)
        geo = dict(stride=(s,) * 3, dilation=(d,) * 3, padding=(d,) * 3, act_out=hip.ACT_RELU)
        w3, wh = hip.pack_weights_bf16(w, split3=True), hip.pack_weights_f16x2(w)
        r3 = rounds(lambda: hip.conv3d_bf16(x, w3, bias, cout, (3, 3, 3), out, split3=True, **geo), 50)
        rh = rounds(lambda: hip.conv3d_bf16(x, wh, bias, cout, (3, 3, 3), out, f16x2=True, **geo), 50)
        report(f"{cin}>{cout} k333 s{s} d{d} @{'x'.join(map(str, dims))}", n, r3, rh, tot)
    taps = ([1], [2, 0])
    for cin, cout, dims, n in PHASES:
        x = hip.Vox.from_ncdhw(torch.randn(1, cin, *dims, device=dev))
        w = torch.randn(cout, cin, 3, 3, 3, device=dev) / (cin * 27) ** 0.5
        bias = torch.randn(cout, device=dev)
        out = hip.Vox.empty(1, tuple(2 * m for m in dims), cout, dev)
        res = hip.Vox.from_ncdhw(torch.randn(1, cout, *(2 * m for m in dims), device=dev))
        p3, ph = [], []
        for px in (0, 1):
            for py in (0, 1):
                for pz in (0, 1):
                    sub = w[:, :, taps[px]][:, :, :, taps[py]][:, :, :, :, taps[pz]].contiguous()
                    p3.append((hip.pack_weights_bf16(sub, split3=True), tuple(sub.shape[2:]), (px, py, pz)))
                    ph.append((hip.pack_weights_f16x2(sub), tuple(sub.shape[2:]), (px, py, pz)))
        kw = dict(res1=res, act_out=hip.ACT_RELU, out_pos=x.dims, o_stride=(2, 2, 2))
        iters = 50 if dims[0] <= 64 else 20
        r3 = rounds(lambda: hip.conv3d_phases(x, p3, bias, cout, out, split3=True, **kw), iters)
        rh = rounds(lambda: hip.conv3d_phases(x, ph, bias, cout, out, f16x2=True, **kw), iters)
        report(f"{cin}>{cout} k333 s2 transposed, 8 phases @{'x'.join(map(str, dims))}", n, r3, rh, tot)
    print(f"per frame (launch counts applied): bf16x3 {tot[0]:.3f} ms, f16x2 {tot[1]:.3f} ms, difference {tot[0] - tot[1]:.3f} ms")


if __name__ == "__main__":
    main()
