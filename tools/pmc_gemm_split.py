"""The two weight images of the pre-split 2-D GEMMs in isolation for rocprofv3 --pmc passes (one pass per counter set, nothing
else traced): one few-pixel K16p launch (2304 x 468 x 384, batch 2) and one chip-filling K16 launch on the A image
(5760 x 1848 x 1280, batch 2), bf16x3 (six bf16 MFMAs per K step) then f16x2 (three fp16 MFMAs), three launches each.
    rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d out -- python tools/pmc_gemm_split.py
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d out -- python tools/pmc_gemm_split.py
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d out -- python tools/pmc_gemm_split.py
    python tools/pmc_table.py out/.../*counter_collection.csv --match gemm_x3
The template arguments tell the rows apart: gemm_x3_panel_kernel<1, 1, 1> / <1, 1, 1, 2> few pixels,
gemm_x3_kernel<2, 2, 4, 2, 1, 3, 1> / <..., 1, 2, 1> chip-filling."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

torch.manual_seed(0)
dev = "cuda"
for M, N, K in ((2304, 468, 384), (5760, 1848, 1280)):
    w = torch.randn(M, K, device=dev) / K ** 0.5
    b = torch.randn(2, K, N, device=dev)
    bias = torch.randn(M, device=dev)
    out = hip.padded_rows((2, M, N), dev)
    for pa in (hip.GemmPacked(w, "a"), hip.GemmPacked(w, "a", split="f16x2")):
        for _ in range(3):
            hip.gemm_x3(pa, b, bias=bias, act="swish", out=out)
torch.cuda.synchronize()
print("done")
