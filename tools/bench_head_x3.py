"""A/B of the full-resolution head convolution (32 -> 32, 3x3x3 @ 256x256x32, dilation 1 / 2 / 3) in isolation (dev tool; GPU):
  K2s   conv3d_c32_slide_kernel      exact fp32 MFMA (v_mfma_f32_32x32x2_f32)
  K2s3  conv3d_c32_slide_x3_kernel   3-way bf16 split in the sliding window (six v_mfma_f32_32x32x16_bf16 per K step)
  K2b3  conv3d_bf16_kernel<SPLIT=3>  the same split in the generic skeleton (round 3's experiment; forced by a tile hint)
with no / one / two residual operands, plus the error of each against ATen float64 on a 16-plane slab of the same data.

    python tools/bench_head_x3.py
    python tools/bench_head_x3.py --lo-ab     K2s3h only: lo weights through the L2 ring (hip.set_head_lo(0)) against resident in
                                              LDS (1, the default), the five (D, NRES) launches of the frame and 32 -> 22; best of
                                              three interleaved rounds and their spread, outputs compared bit for bit
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from occdepth_amd import hip
from bench_kernels import time_many

DIMS = (256, 256, 32)
GFLOP = 2.0 * DIMS[0] * DIMS[1] * DIMS[2] * 27 * 32 * 32 / 1e9


def main():
    torch.manual_seed(0)
    x = hip.Vox(torch.randn(1, *DIMS, 32, device="cuda"), 32)
    r1 = hip.Vox(torch.randn(1, *DIMS, 32, device="cuda"), 32)
    r2 = hip.Vox(torch.randn(1, *DIMS, 32, device="cuda"), 32)
    out = hip.Vox.empty(1, DIMS, 32, "cuda")
    w = torch.randn(32, 32, 3, 3, 3, device="cuda") / (32 * 27) ** 0.5
    bias = torch.randn(32, device="cuda")
    w32, w3 = hip.pack_weights(w), hip.pack_weights_bf16(w, split3=True)
    for d in (1, 2, 3):
        geo = dict(dilation=(d,) * 3, padding=(d,) * 3)
        for nres, kw in ((0, {}), (1, dict(res1=r1, act_out=hip.ACT_RELU)), (2, dict(res1=r1, res2=r2, act_in=hip.ACT_RELU,
                                                                                       act_out=hip.ACT_RELU))):
            fns = {
                "K2s  fp32": lambda: hip.conv3d(x, w32, bias, 32, (3, 3, 3), out, **geo, **kw),
                "K2s3 bf16x3 slide": lambda: hip.conv3d_bf16(x, w3, bias, 32, (3, 3, 3), out, split3=True, **geo, **kw),
            }
            if nres == 0:
                fns["K2b3 bf16x3 generic"] = lambda: hip.conv3d_bf16(x, w3, bias, 32, (3, 3, 3), out, split3=True, tile_hint=2,
                                                                      **geo, **kw)
            ms = time_many(fns, rounds=5, iters=6)
            for name, t in ms.items():
                issued = 6.0 if "x3" in name else 1.0
                peak = 2500.0 if "x3" in name else 157.3
                print(f"head d={d} nres={nres} {name:20s}: {t:7.4f} ms  {GFLOP / t:7.1f} TF/s algorithmic  "
                      f"{issued * GFLOP / t:7.1f} TF/s issued = {issued * GFLOP / t / peak * 100:5.1f} % of the {peak:.1f} TF/s pipe peak",
                      flush=True)
    # accuracy on a 16-plane slab of the same data (float64 on the CPU)
    xs = hip.Vox(x.buf[:, :16].contiguous(), 32)
    ref_in = xs.ncdhw().cpu().double()
    for d in (1, 2, 3):
        ref = F.conv3d(ref_in, w.cpu().double(), bias.cpu().double(), padding=d, dilation=d)
        o = hip.Vox.empty(1, (16, 256, 32), 32, "cuda")
        for name, fn in (("K2s  fp32", lambda: hip.conv3d(xs, w32, bias, 32, (3, 3, 3), o, dilation=(d,) * 3, padding=(d,) * 3)),
                         ("K2s3 bf16x3 slide", lambda: hip.conv3d_bf16(xs, w3, bias, 32, (3, 3, 3), o, dilation=(d,) * 3,
                                                                        padding=(d,) * 3, split3=True))):
            fn()
            got = o.ncdhw().cpu().double()
            print(f"error d={d} {name:20s}: max |delta| / max |ref| {float((got - ref).abs().max() / ref.abs().max()):.3e}   "
                  f"rms rel {float((got - ref).norm() / ref.norm()):.3e}", flush=True)


def lo_ab(rounds=3, iters=10):
    torch.manual_seed(0)
    x = hip.Vox(torch.randn(1, *DIMS, 32, device="cuda"), 32)
    r1 = hip.Vox(torch.randn(1, *DIMS, 32, device="cuda"), 32)
    r2 = hip.Vox(torch.randn(1, *DIMS, 32, device="cuda"), 32)
    bias = torch.randn(32, device="cuda")
    cases = [(1, 0, 32), (2, 0, 32), (3, 0, 32), (2, 1, 32), (3, 2, 32), (1, 0, 22)]
    epi = {0: {}, 1: dict(res1=r1, act_out=hip.ACT_RELU), 2: dict(res1=r1, res2=r2, act_in=hip.ACT_RELU, act_out=hip.ACT_RELU)}
    print(f"# K2s3h, 32 -> cout 3x3x3 @ {DIMS}, N(0,1) data; ms per launch: best of {rounds} rounds of {iters} launches "
          f"(spread = max - min of the rounds), ring = set_head_lo(0), lds = set_head_lo(1)")
    for d, nres, cout in cases:
        w = torch.randn(cout, 32, 3, 3, 3, device="cuda") / (32 * 27) ** 0.5
        wpk = hip.pack_weights_f16x2(w)
        out = hip.Vox.empty(1, DIMS, cout, "cuda")
        run = lambda: hip.conv3d_f16x2(x, wpk, bias, cout, (3, 3, 3), out, dilation=(d,) * 3, padding=(d,) * 3, **epi[nres])
        ms, bits = {0: [], 1: []}, {}
        for form in (0, 1):
            old = hip.set_head_lo(form)
            try:
                run()
                torch.cuda.synchronize()
                bits[form] = out.buf.clone()
            finally:
                hip.set_head_lo(old)
        for _ in range(rounds):
            for form in (0, 1):
                old = hip.set_head_lo(form)
                try:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        run()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[form].append(e0.elapsed_time(e1) / iters)
                finally:
                    hip.set_head_lo(old)
        b0, b1 = min(ms[0]), min(ms[1])
        print(f"head 32>{cout} d={d} nres={nres}: ring {b0:.4f} ms (spread {max(ms[0]) - b0:.4f})  lds {b1:.4f} ms "
              f"(spread {max(ms[1]) - b1:.4f})  delta {1e3 * (b1 - b0):+.1f} us  {b0 / b1:.3f}x  "
              f"bit-identical {torch.equal(bits[0], bits[1])}", flush=True)


if __name__ == "__main__":
    lo_ab() if "--lo-ab" in sys.argv[1:] else main()
