"""The split head kernels in isolation (32 -> 32, 3x3x3 @ 256x256x32, dilation 1, no residual) for rocprofv3 --pmc passes:
K2s3 (bf16x3, six bf16 MFMAs per K step) and K2s3h (f16x2, three fp16 MFMAs per K step) in both of its forms -- lo weights
through the L2 ring (hip.set_head_lo(0), instantiation <..., false>) and resident in LDS (1, <..., true>) -- three launches each.
    rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d out -- python tools/pmc_head_split.py
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d out -- python tools/pmc_head_split.py
    python tools/pmc_table.py out/.../*counter_collection.csv --match slide
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

torch.manual_seed(0)
dims = (256, 256, 32)
x = hip.Vox(torch.randn(1, *dims, 32, device="cuda"), 32)
w = torch.randn(32, 32, 3, 3, 3, device="cuda") / (32 * 27) ** 0.5
bias = torch.zeros(32, device="cuda")
out = hip.Vox.empty(1, dims, 32, "cuda")
geo = dict(dilation=(1, 1, 1), padding=(1, 1, 1))
w3, wh = hip.pack_weights_bf16(w, split3=True), hip.pack_weights_f16x2(w)
for _ in range(3):
    hip.conv3d_bf16(x, w3, bias, 32, (3, 3, 3), out, split3=True, **geo)
for form in (0, 1):
    old = hip.set_head_lo(form)
    for _ in range(3):
        hip.conv3d_f16x2(x, wh, bias, 32, (3, 3, 3), out, **geo)
    hip.set_head_lo(old)
torch.cuda.synchronize()
print("done")
