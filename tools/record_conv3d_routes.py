"""Which kernel the eval-path 3-D convolutions take, for every switch setting, as a table (tests/golden/conv3d_routes.json).

    python tools/record_conv3d_routes.py --device cpu  --out tests/golden/conv3d_routes.json
    python tools/record_conv3d_routes.py --device cuda --out tests/golden/conv3d_routes.json     (adds its section)

The plans of occdepth_amd.fused are driven over a fixed list of cases (CASES) crossed with the switches (settings());
hip.conv3d / conv3d_bf16 / conv3d_f16x2 / conv3d_phases and the three weight packers are replaced by recorders that launch
nothing, so a run touches the device only for allocations and the finite-weights test of the fp16 image.  Per case and setting
the table holds the sequence of launches: entry point, split3 / f16x2 flag, weight image kind, kernel extent, o_off and the
number of merged phases.  tests/test_conv3d_routes.py replays the cases and requires equal sequences; the committed table was
recorded before the dispatch was rewritten around fused.route().
"""
import argparse
import contextlib
import itertools
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from occdepth_amd import fused, hip  # noqa: E402

PACKERS = {"pack_weights": ("f32", torch.float32), "pack_weights_bf16": ("bf16", torch.bfloat16),
           "pack_weights_f16x2": ("f16x2", torch.uint8)}
LAUNCHERS = ("conv3d", "conv3d_bf16", "conv3d_f16x2", "conv3d_phases")


def _digits(t):
    return "".join(str(int(v)) for v in t)


@contextlib.contextmanager
def stubbed(log, packs=None):
    """hip's 3-D launchers and packers replaced: launches append one line to `log`, packs (kind) to `packs`."""
    saved = {n: getattr(hip, n) for n in LAUNCHERS + tuple(PACKERS)}

    def packer(name):
        kind, dtype = PACKERS[name]

        def pack(w, scale=None, layout=0, split3=False):
            img = torch.empty(0, dtype=dtype, device=w.device)
            img.kind = "x3" if split3 else kind
            if packs is not None:
                packs.append(img.kind)
            return img
        return pack

    def flags(kw):
        return "split3" if kw.get("split3") else "f16x2" if kw.get("f16x2") else "-"

    def launcher(name):
        def launch(x, wpk, bias, cout, kernel, out, **kw):
            log.append(f"{name} {flags(kw)} {wpk.kind} k{_digits(kernel)} o{_digits(kw.get('o_off', (0, 0, 0)))}")
            return out
        return launch

    def phases(x, phases, bias, cout, out, **kw):
        per = ",".join(f"{wpk.kind}:k{_digits(kern)}:o{_digits(off)}" for wpk, kern, off in phases)
        log.append(f"conv3d_phases {flags(kw)} n{len(phases)} {per}")
        return out

    try:
        for name in PACKERS:
            setattr(hip, name, packer(name))
        for name in LAUNCHERS[:3]:
            setattr(hip, name, launcher(name))
        hip.conv3d_phases = phases
        yield
    finally:
        for n, f in saved.items():
            setattr(hip, n, f)


def settings(transposed=False):
    """[(label, dict)]: the cross of the switches (BF16X3_DILATED under "all" only; PHASES_* for the transposed plans only)."""
    out = []
    for x3, head, k2b, sv, k1 in itertools.product((False, "head", "all"), ("f16x2", "bf16x3"), ("f16x2", "bf16x3"), (True, False),
                                                  (False, True)):
        for dil in ((False, True) if x3 == "all" else (False,)):
            for one, px3 in (itertools.product((True, False), (True, False)) if transposed else ((True, True),)):
                s = dict(BF16X3=x3, HEAD_SPLIT=head, K2B_SPLIT=k2b, BF16X3_SMALLVOL=sv, BF16X3_DILATED=dil, PHASES_ONE_LAUNCH=one,
                         PHASES_X3=px3, SMALLVOL_KERNELS=((3, 3, 3), (1, 1, 1)) if k1 else ((3, 3, 3),))
                label = f"x3={x3 or 'off'} head={head} k2b={k2b} sv={int(sv)} k1={int(k1)} dil={int(dil)}"
                out.append((label + (f" one={int(one)} px3={int(px3)}" if transposed else ""), s))
    return out


SWITCHES = ("BF16X3", "HEAD_SPLIT", "K2B_SPLIT", "BF16X3_SMALLVOL", "BF16X3_DILATED", "PHASES_ONE_LAUNCH", "PHASES_X3", "SMALLVOL_KERNELS")


@contextlib.contextmanager
def switches(s):
    saved = {n: getattr(fused, n) for n in SWITCHES}
    try:
        apply_switches(s)
        yield
    finally:
        apply_switches(saved)


def apply_switches(s):
    fused.set_bf16x3(s["BF16X3"])
    fused.set_head_split(s["HEAD_SPLIT"])
    fused.set_k2b_split(s["K2B_SPLIT"])
    for n in SWITCHES[3:]:
        setattr(fused, n, s[n])


def _conv(cin, cout, dims, k=3, dilation=1, act_in=0, cs=None, coff=0, inf=False, hint=0, kind="conv"):
    return dict(kind=kind, cin=cin, cout=cout, dims=dims, k=k, dilation=dilation, act_in=act_in, cs=cs, coff=coff, inf=inf, hint=hint)


BIG, HALF, Z16, SMALL = (64, 64, 32), (32, 64, 32), (64, 64, 16), (8, 8, 4)
CASES = {}
for _d in (1, 2, 3):
    CASES[f"head_32_32_d{_d}_512tiles"] = _conv(32, 32, BIG, dilation=_d)
    CASES[f"head_32_32_d{_d}_256tiles"] = _conv(32, 32, HALF, dilation=_d)
    CASES[f"head_32_32_d{_d}_z16"] = _conv(32, 32, Z16, dilation=_d)
CASES.update({
    "head_25_20": _conv(25, 20, BIG),
    "head_24_32": _conv(24, 32, BIG),
    "head_32_32_relu": _conv(32, 32, BIG, act_in=hip.ACT_RELU),
    "head_32_32_inf_weight": _conv(32, 32, BIG, inf=True),
    "head_derived": _conv(32, 32, BIG, kind="derived"),
    "small_128_128": _conv(128, 128, SMALL),
    "small_128_128_d2": _conv(128, 128, SMALL, dilation=2),
    "small_136_128": _conv(136, 128, SMALL),
    "small_128_128_9216vox": _conv(128, 128, (32, 32, 9)),
    "small_128_128_k1": _conv(128, 128, SMALL, k=1),
    "small_128_128_relu": _conv(128, 128, SMALL, act_in=hip.ACT_RELU),
    "small_128_128_sigmoid": _conv(128, 128, SMALL, act_in=hip.ACT_SIGMOID),
    "small_128_128_k1_sigmoid": _conv(128, 128, SMALL, k=1, act_in=hip.ACT_SIGMOID),
    "small_128_128_cs132": _conv(128, 128, SMALL, cs=132),
    "small_128_128_coff4": _conv(128, 128, SMALL, cs=136, coff=4),
    "small_128_128_tile_hint": _conv(128, 128, SMALL, hint=3),
    "small_128_128_inf_weight": _conv(128, 128, SMALL, inf=True),
    "small_128_64": _conv(128, 64, SMALL),
    "small_derived": _conv(128, 128, SMALL, kind="derived"),
    "mid_64_64": _conv(64, 64, (32, 32, 8)),
    "mid_64_64_d2": _conv(64, 64, (32, 32, 8), dilation=2),
    "mid_64_64_k1": _conv(64, 64, (32, 32, 8), k=1),
    "mid_64_64_cs68": _conv(64, 64, (32, 32, 8), cs=68),
    "mid_64_64_sigmoid": _conv(64, 64, (32, 32, 8), act_in=hip.ACT_SIGMOID),
    "convt_s2_64_32": _conv(64, 32, (4, 4, 2), kind="convt2"),
    "convt_s2_128_64": _conv(128, 64, (4, 4, 2), kind="convt2"),
    "convt_s2_128_64_inf_weight": _conv(128, 64, (4, 4, 2), kind="convt2", inf=True),
    "convt_s2_12_8": _conv(12, 8, (4, 4, 2), kind="convt2"),
    "convt_s2_12_8_cs12": _conv(12, 8, (4, 4, 2), kind="convt2", cs=12),
    "convt_s1_32_32": _conv(32, 32, BIG, kind="convt1"),
    "rows_128_128": _conv(128, 128, SMALL, kind="rows"),
    "rows_128_128_sigmoid": _conv(128, 128, SMALL, kind="rows", act_in=hip.ACT_SIGMOID),
    "rows_128_128_prepacked_twice": _conv(128, 128, SMALL, kind="rows_packed", act_in=hip.ACT_SIGMOID),
})


def _vox(c, device):
    cs = c["cs"] if c["cs"] is not None else hip.round_up(c["cin"], 8)
    return hip.Vox(torch.empty((1,) + tuple(c["dims"]) + (cs,), device=device), c["cin"], c["coff"])


def build_case(c, device):
    """The modules of a case (built once, shared by all its settings) -> a function that makes a fresh plan and calls it."""
    torch.manual_seed(0)
    k, d = c["k"], c["dilation"]
    pad = d * (k // 2)
    x = _vox(c, device)
    with torch.no_grad():
        if c["kind"] in ("rows", "rows_packed"):
            b = torch.randn(c["cin"], c["cout"], device=device)
            out = hip.Vox.empty(1, c["dims"], c["cout"], device)
            if c["kind"] == "rows":
                return lambda: fused.gemm_rows(x, b, out, act_in=c["act_in"])

            def twice():
                packed = fused.pack_rows(b)
                fused.gemm_rows(x, packed, out, act_in=c["act_in"])
                fused.gemm_rows(x, packed, out, act_in=c["act_in"])
            return twice
        if c["kind"] in ("convt1", "convt2"):
            up = 2 if c["kind"] == "convt2" else 1
            mod = nn.ConvTranspose3d(c["cin"], c["cout"], 3, stride=up, padding=1, output_padding=up - 1).to(device)
            bn = nn.BatchNorm3d(c["cout"]).to(device).eval()
            if c["inf"]:
                mod.weight[1, 2, 1, 1, 1] = float("inf")
            return lambda: fused.ConvTransposePlan(mod, bn)(x, act_out=hip.ACT_RELU)
        mod = nn.Conv3d(c["cin"], c["cout"], k, padding=pad, dilation=d, bias=False).to(device)
        bn = nn.BatchNorm3d(c["cout"]).to(device).eval()
        if c["inf"]:
            mod.weight[1, 2, 0, 0, 0] = float("inf")
        if c["kind"] == "derived":
            return lambda: fused.DerivedConvPlan([mod], lambda: (mod.weight, None), padding=(pad,) * 3, dilation=(d,) * 3)(
                x, act_in=c["act_in"])
        if c["hint"]:
            def hinted():          # (no plan passes tile_hint: the launch helper directly, on the plan's operands)
                plan = fused.ConvPlan(mod, bn)
                plan._prepare()
                kk, s, dd, p = plan.geometry()
                out = hip.Vox.empty(1, plan.out_dims(x.dims), plan.cout, device)
                fused._conv3d(x, plan._wpk, plan._bias, plan.cout, kk, out, stride=s, dilation=dd, padding=p, tile_hint=c["hint"])
            return hinted
        return lambda: fused.ConvPlan(mod, bn)(x, act_in=c["act_in"])


def record(device, names=None):
    """{case: [launch sequence per setting, in settings() order]} on `device`."""
    table = {}
    for name, c in CASES.items():
        if names is not None and name not in names:
            continue
        run = build_case(c, device)
        rows = []
        for _, s in settings(transposed=c["kind"] == "convt2"):
            log = []
            with switches(s), stubbed(log), torch.no_grad():
                run()
            rows.append(log)
        table[name] = rows
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", choices=("cpu", "cuda"), required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    table = record(a.device)
    # the sequences repeat: store each distinct one once and the table as indices into that list
    seqs = doc.setdefault("sequences", [])
    index = {json.dumps(s): i for i, s in enumerate(seqs)}
    section = {}
    for name, rows in table.items():
        ids = []
        for log in rows:
            key = json.dumps(log)
            if key not in index:
                index[key] = len(seqs)
                seqs.append(log)
            ids.append(index[key])
        section[name] = ids
    doc[a.device] = section
    doc["settings"] = [label for label, _ in settings()]
    doc["settings_transposed"] = [label for label, _ in settings(transposed=True)]
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{a.device}: {len(section)} cases, {sum(len(v) for v in section.values())} rows, {len(seqs)} distinct sequences -> {a.out}")


if __name__ == "__main__":
    main()
