"""K2b's two splits in isolation for rocprofv3 --pmc passes (one pass per counter set, nothing else traced): the 256 -> 256
3x3x3 dilation-1 small-volume launch @32x32x4 (variant 8, in-workgroup split-K) and the merged 64 -> 32 phase launch
@128x128x16, bf16x3 (six bf16 MFMAs per K step) then f16x2 (K2bh: three fp16 MFMAs), three launches each.
    rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d out -- python tools/pmc_k2b_split.py
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d out -- python tools/pmc_k2b_split.py
    rocprofv3 --pmc WRITE_SIZE --output-format csv -d out -- python tools/pmc_k2b_split.py
    python tools/pmc_table.py out/.../*counter_collection.csv --match conv3d_bf16_kernel
The template arguments tell the rows apart: <1, 1, 1, 4, ..., 3, 4> / <..., 2, 4> small volume, <..., 3, 1> / <..., 2, 1> phases."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

torch.manual_seed(0)
dev = "cuda"
x = hip.Vox.from_ncdhw(torch.randn(1, 256, 32, 32, 4, device=dev))
w = torch.randn(256, 256, 3, 3, 3, device=dev) / (256 * 27) ** 0.5
bias = torch.zeros(256, device=dev)
out = hip.Vox.empty(1, (32, 32, 4), 256, dev)
geo = dict(dilation=(1, 1, 1), padding=(1, 1, 1))
w3, wh = hip.pack_weights_bf16(w, split3=True), hip.pack_weights_f16x2(w)
for _ in range(3):
    hip.conv3d_bf16(x, w3, bias, 256, (3, 3, 3), out, split3=True, **geo)
for _ in range(3):
    hip.conv3d_bf16(x, wh, bias, 256, (3, 3, 3), out, f16x2=True, **geo)

xp = hip.Vox.from_ncdhw(torch.randn(1, 64, 128, 128, 16, device=dev))
wp = torch.randn(32, 64, 3, 3, 3, device=dev) / (64 * 27) ** 0.5
bp = torch.zeros(32, device=dev)
outp = hip.Vox.empty(1, (256, 256, 32), 32, dev)
taps = ([1], [2, 0])
p3, ph = [], []
for px in (0, 1):
    for py in (0, 1):
        for pz in (0, 1):
            sub = wp[:, :, taps[px]][:, :, :, taps[py]][:, :, :, :, taps[pz]].contiguous()
            p3.append((hip.pack_weights_bf16(sub, split3=True), tuple(sub.shape[2:]), (px, py, pz)))
            ph.append((hip.pack_weights_f16x2(sub), tuple(sub.shape[2:]), (px, py, pz)))
kw = dict(out_pos=xp.dims, o_stride=(2, 2, 2))
for _ in range(3):
    hip.conv3d_phases(xp, p3, bp, 32, outp, split3=True, **kw)
for _ in range(3):
    hip.conv3d_phases(xp, ph, bp, 32, outp, f16x2=True, **kw)
torch.cuda.synchronize()
print("done")
