"""Cost of the Lovasz-softmax loss (csrc/lovasz.hip) and of the sort under it (K38, csrc/sort.hip) on a config-2 frame:
256 x 256 x 32 voxels x 20 classes, B = 1 -- 20 segments of 2 M (key, value) pairs, 4 passes of 8 bits over the 31 key bits.
The scene is bench_visibility.py's synthetic street turned into logits (6 on the labelled class plus unit noise).  It times

    errors         occd_lovasz_errors (streaming), both layouts
    sort           occd_sort_pairs_u32 behind it; per pass, against the minimal traffic of a pass (keys + values read by the
                   histogram launch -- keys only -- and by the scatter launch, written once: 20 bytes a pair), and the three
                   launches of a pass by the library's own event pairs
    ranks          occd_lovasz_ranks on the sorted pairs
    backward       occd_lovasz_bwd (streaming)
    torch          the package's torch formulation (torch.sort per class) on the GPU, forward + backward, the A/B baseline

    python tools/bench_lovasz.py [--rounds 7] [--iters 10] [--out profiles/lovasz_ab.txt]

The training-step and forward-frame lines at the end of the committed profile are bench.py runs of the same session (fresh
processes of the parent commit and of this tree in turn), added by hand, as is the note in parentheses under the gradient line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_map import C, DIMS, interleaved  # noqa: E402
from bench_visibility import street  # noqa: E402
from occdepth_amd import hip  # noqa: E402
from occdepth_amd.loss import lovasz_loss as ll  # noqa: E402


COPY_TBPS = 6.3          # what a plain float4 copy reaches on an MI355X (8.0 TB/s is the specification)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per window of the device-event timings")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "lovasz_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lovasz.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    N = X * Y * Z
    target = torch.from_numpy(street(DIMS)).to(dev)[None].contiguous()
    g = torch.Generator(device="cuda").manual_seed(0)
    lab = torch.where(target == 255, torch.zeros_like(target), target).long()
    logits = torch.randn((1, C, X, Y, Z), device=dev, generator=g)
    logits.scatter_add_(1, lab[:, None], torch.full((1, 1, X, Y, Z), 6.0, device=dev))
    rows = torch.zeros((1, X, Y, Z, 24), device=dev)                        # the 3-D stack's channels-last rows, cs = 24
    rows[..., :C] = logits.permute(0, 2, 3, 4, 1)
    logits_cl = rows[..., :C].permute(0, 4, 1, 2, 3)

    sc = hip.lovasz_scratch(N, C, logits.device)                             # the one the loss itself will use
    pairs = sc["pairs"]
    passes = hip.sort_passes(0, hip.LOVASZ_KEY_BITS)

    def errors(z=logits_cl):
        hip.lovasz_errors(z, target, 0, C, pairs[0, 0], pairs[0, 1])

    def errors_sort():
        errors()
        return hip.sort_pairs(pairs[0, 0], pairs[0, 1], 0, hip.LOVASZ_KEY_BITS, (pairs[1, 0], pairs[1, 1], sc["hist"]))

    def forward():
        return hip.lovasz_forward(logits_cl, target)

    q, fg_count, loss_q = forward()
    gscale = torch.full((1,), 1.0 / C, device=dev)
    res = interleaved({"errors_planes": lambda: errors(logits), "errors_rows": errors, "errors_sort": errors_sort,
                       "forward": forward, "bwd": lambda: hip.lovasz_bwd(logits_cl, target, q, gscale)}, args.rounds, args.iters)
    torch.cuda.synchronize()
    with hip.profile() as prof:
        for _ in range(args.iters):
            forward()
    tags = ("lovasz_errors", "sort_hist", "sort_scan", "sort_scatter", "lovasz_ranks")
    by_tag = {t: prof.rows[t]["ms"] / args.iters for t in tags}
    sort_ms = res["errors_sort"][0] - res["errors_rows"][0]
    ranks_ms = res["forward"][0] - res["errors_sort"][0]
    n_pairs = C * N
    gb_pass = n_pairs * 20.0 / 1e9
    present = int((fg_count > 0).sum())
    lines = ["Lovasz-softmax loss on the K38 sort, %d x %d x %d voxels x %d classes, B = 1: %d segments of %d pairs, %d passes of %d bits;"
             % (X, Y, Z, C, C, N, passes, hip.SORT_RADIX_BITS),
             "ms per call, median (min) over %d rounds of %d calls (device events; the variants alternate inside every round);"
             % (args.rounds, args.iters), "tools/bench_lovasz.py", "",
             "scene: a synthetic street, %d of %d classes present, %.1f %% of the voxels unknown" % (present, C, 100.0 * float((target == 255).float().mean())),
             "occd_lovasz_errors     channels-last rows (cs 24) %8.4f (%.4f) ms; planes %8.4f (%.4f) ms  (reads %d MB, writes %d MB)"
             % (res["errors_rows"] + res["errors_planes"] + (N * (4 * C + 1) // 1000000, n_pairs * 8 // 1000000)),
             "occd_sort_pairs_u32    %8.4f ms (errors + sort %.4f (%.4f) less the errors pass) = %.4f ms a pass: %.2f TB/s against the"
             % (sort_ms, res["errors_sort"][0], res["errors_sort"][1], sort_ms / passes, gb_pass / (sort_ms / passes)),
             "                       %.2f GB a pass must move (%d M pairs: keys read twice, values read once, both written once)"
             % (gb_pass, n_pairs // 1000000),
             "                       (bandwidth-bound; %.0f %% of the %.1f TB/s a plain float4 copy reaches on an MI355X)"
             % (100.0 * gb_pass / (sort_ms / passes) / COPY_TBPS, COPY_TBPS),
             "   a pass by the library's own event pairs (mean of %d calls): histograms %.4f + scan %.4f + scatter %.4f ms"
             % (args.iters, by_tag["sort_hist"] / passes, by_tag["sort_scan"] / passes, by_tag["sort_scatter"] / passes),
             "   the %s launch bounds a pass" % max(("sort_hist", "sort_scan", "sort_scatter"), key=lambda t: by_tag[t])[5:],
             "occd_lovasz_ranks      %8.4f ms (forward %.4f (%.4f) less errors + sort); by its event pair %.4f ms"
             % (ranks_ms, res["forward"][0], res["forward"][1], by_tag["lovasz_ranks"]),
             "occd_lovasz_bwd        %8.4f (%.4f) ms" % res["bwd"],
             "scratch: %d bytes (%.1f MiB) cached per (N, class group); with class_chunk = 5: %.1f MiB; q, the forward's saved state: %.1f MiB"
             % (hip.lovasz_scratch_bytes(N, C), hip.lovasz_scratch_bytes(N, C) / 2 ** 20, hip.lovasz_scratch_bytes(N, C, 5) / 2 ** 20,
                N * C * 4 / 2 ** 20)]

    # the whole loss, forward + backward through autograd, kernels against the torch formulation on the GPU
    leaf = rows.clone().requires_grad_(True)
    fn = ll.LovaszSoftmaxLoss()
    chunked = ll.LovaszSoftmaxLoss(class_chunk=5)

    def hip_loss(f=fn):
        leaf.grad = None
        f(leaf[..., :C].permute(0, 4, 1, 2, 3), target).backward()

    def torch_loss():
        leaf.grad = None
        ll.lovasz_softmax_torch(leaf[..., :C].permute(0, 4, 1, 2, 3), target).backward()

    whole = interleaved({"hip": hip_loss, "chunked": lambda: hip_loss(chunked), "torch": torch_loss}, args.rounds, 3)
    hip_loss()
    g_hip = leaf.grad.clone()
    l_hip = float(fn(leaf[..., :C].permute(0, 4, 1, 2, 3), target).detach())
    torch_loss()
    l_torch = float(ll.lovasz_softmax_torch(leaf[..., :C].permute(0, 4, 1, 2, 3), target).detach())
    g_torch = leaf.grad.clone()
    leaf64 = rows.double().requires_grad_(True)                              # the yardstick of both: the same formulation in float64
    l64 = ll.lovasz_softmax_torch(leaf64[..., :C].permute(0, 4, 1, 2, 3), target)
    l64.backward()
    top = float(leaf64.grad.abs().max())
    e_hip, e_torch = float((g_hip - leaf64.grad).abs().max()) / top, float((g_torch - leaf64.grad).abs().max()) / top
    lines += ["",
              "the whole loss, forward + backward through autograd (host enqueue included):",
              "  kernels %8.4f (%.4f) ms; class_chunk = 5 %8.4f (%.4f) ms; torch formulation on the GPU %8.2f (%.2f) ms (%.1fx);"
              % (whole["hip"] + whole["chunked"] + whole["torch"] + (whole["torch"][0] / whole["hip"][0],)),
              "  loss %.7f / %.7f (float64 torch: %.9f); gradient max|delta| / max against float64 torch: kernels %.2e, float32 torch %.2e"
              % (l_hip, l_torch, float(l64.detach()), e_hip, e_torch),
              "pruning the background voxels below the smallest foreground error (their g is 0): not tried.",
              "",
              "the effect of the loss on mIoU is not measured: no checkpoint and no dataset where this was run."]
    result = {"errors_ms": round(res["errors_rows"][0], 4), "sort_ms": round(sort_ms, 4), "ranks_ms": round(ranks_ms, 4),
              "bwd_ms": round(res["bwd"][0], 4), "whole_ms": round(whole["hip"][0], 4), "torch_ms": round(whole["torch"][0], 2),
              "pass_tbps": round(gb_pass / (sort_ms / passes), 3)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
