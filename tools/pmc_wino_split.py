"""The fused Winograd kernels in isolation on the 80 -> 80 level (2 x 370 x 1220, LeakyReLU) for rocprofv3 --pmc passes: K10
(fp32 MFMA) and K10h (the two-term fp16 split), three launches each.
    rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d out -- python tools/pmc_wino_split.py
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d out -- python tools/pmc_wino_split.py
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d out -- python tools/pmc_wino_split.py
(FETCH_SIZE and WRITE_SIZE do not fit into one pass: rocprofv3 refuses the configuration.)
    python tools/pmc_table.py out/.../*counter_collection.csv --match wino3x3
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

torch.manual_seed(0)
cin = cout = 80
x = torch.randn(2, cin, 370, 1220, device="cuda")
w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.1
sc, sh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda")
y = torch.empty(2, cout, 370, 1220, device="cuda")
for upk in (hip.wino_pack_weights(w, sc), hip.wino_pack_weights_f16x2(w, sc)):
    for _ in range(3):
        hip.conv2d_3x3_fused(x, upk, cout, sh, "leaky", out=y)
torch.cuda.synchronize()
print("done")
