"""What the four 3-D implicit-GEMM entry points return and launch, as a table (tests/golden/conv3d_codes.json).

    python tools/record_conv3d_codes.py --device cpu  --out tests/golden/conv3d_codes.json     (no GPU in the machine)
    python tools/record_conv3d_codes.py --device cuda --out tests/golden/conv3d_codes.json     (adds its section)

cpu: the host half of csrc/conv3d_igemm.hip and csrc/conv3d_bf16.hip.  BASES crossed with one-field PERTURBATIONS go through
occd_conv3d_fwd, occd_conv3d_fwd_phases, occd_conv3d_bf16_fwd and occd_conv3d_bf16_fwd_phases (CALLS) with placeholder
pointers; without a device a descriptor ends as OCCD_EINVAL (validation), OCCD_ENOMEM (no variant fits) or OCCD_ELAUNCH (it
passed every host check and reached the runtime).  Nothing is dereferenced on the host, but a device would be handed the
placeholders: this section is neither recorded nor replayed where torch.cuda.is_available().
cuda: LAUNCHES on seeded inputs drawn on the CPU; per launch the hip.profile() rows (tag, launches, flops, bytes: the cost
model and the profile names) and the sha256 of the output buffer (which moves when a variant, a tiling or a phase order moves).

tests/test_conv3d_codes.py replays both sections and requires equal tables; the committed one was recorded before the host
halves of the two files were merged into csrc/conv3d_tile.h.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from occdepth_amd import hip  # noqa: E402

# ------------------------------------------------------------------------------------------------- cpu: return codes
PTR = dict(inp=0x10000000, wpk=0x20000000, bias=0x30000000, res1=0x40000000, res2=0x50000000, out=0x60000000)
MAXN = 8


def _r(x, m):
    return (x + m - 1) // m * m


def _desc(cin, cout, dims, k=(3, 3, 3), dil=(1, 1, 1), pad=None, in_cs=None, out_cs=None, up=1, off=(0, 0, 0)):
    """One descriptor as a dict of occd_conv3d_args fields ("same" padding unless given; `up`: the output scatter stride)."""
    pad = tuple(d * (kk // 2) for d, kk in zip(dil, k)) if pad is None else pad
    out_cs = _r(cout, 8) if out_cs is None else out_cs
    d = dict(inp=PTR["inp"], wpk=PTR["wpk"], bias=PTR["bias"], res1=None, res2=None, out=PTR["out"], batch=1,
             cin=cin, in_cs=_r(cin, 8) if in_cs is None else in_cs, in_coff=0, cout=cout, out_cs=out_cs, out_coff=0,
             res1_cs=0, res1_coff=0, res2_cs=0, res2_coff=0, act_in=0, act_out=0, tile_hint=0,
             cout_store=min(_r(cout, 8), out_cs, _r(cout, 32)))
    for ax, i in zip("xyz", range(3)):
        d[ax.upper()] = dims[i]
        d["k" + ax], d["s" + ax], d["d" + ax], d["p" + ax] = k[i], 1, dil[i], pad[i]
        d[ax.upper() + "o"], d["O" + ax.upper()] = dims[i], dims[i] * up
        d["o_stride_" + ax], d["o_off_" + ax] = up, off[i]
    return d


def _same(d):
    return [dict(d) for _ in range(MAXN)]


def _transposed(cin, cout, dims):
    """The 8 sub-pixel phases of a ConvTranspose3d(k3, s2, p1, op1): tap subsets of extent 1 or 2 per axis, padding 0."""
    out = []
    for px in (0, 1):
        for py in (0, 1):
            for pz in (0, 1):
                d = _desc(cin, cout, dims, k=(1 + px, 1 + py, 1 + pz), pad=(0, 0, 0), up=2, off=(px, py, pz))
                d["wpk"] = PTR["wpk"] + 0x100000 * len(out)
                out.append(d)
    return out


# name -> MAXN descriptors (a plain launch: eight copies of one, so that the phase entry points take it with any n)
BASES = {
    "64_64_k3_8x8x8": _same(_desc(64, 64, (8, 8, 8))),
    "40_20_k3_5x3x5_rows40_24": _same(_desc(40, 20, (5, 3, 5), in_cs=40, out_cs=24)),
    "256_256_k3_8x8x4": _same(_desc(256, 256, (8, 8, 4))),
    "convt_64_32_8x8x4": _transposed(64, 32, (8, 8, 4)),
    "convt_32_16_8x8x4": _transposed(32, 16, (8, 8, 4)),           # cin <= 32: K2's phases fall back to single launches
    "slab_over_lds_64_64_d32_4x64x64": _same(_desc(64, 64, (4, 64, 64), dil=(1, 32, 32))),   # > 160 KB for every variant
    "head_32_32_k3_32x128x32": _same(_desc(32, 32, (32, 128, 32))),
}


def _set(**kw):
    return lambda d: d.update(kw)


def _add(**kw):
    return lambda d: d.update({k: (d[k] or 0) + v for k, v in kw.items()})


def _with_res(which, then=None):
    def f(d):
        for r in which:
            d[r], d[r + "_cs"] = PTR[r], d["out_cs"]
        if then is not None:
            then(d)
    return f


def perturbations():
    """[(name, scope, f)]: f edits one descriptor dict in place; scope "all" = every phase, "one" = phase 1 only."""
    p = [("base", "all", lambda d: None)]
    for f in ("batch", "X", "Y", "Z", "cin", "cout", "kx", "ky", "kz", "sx", "sy", "sz", "Xo", "Yo", "Zo"):
        p += [(f"{f}=0", "all", _set(**{f: 0})), (f"{f}=-1", "all", _set(**{f: -1}))]
    for t in ("in", "out", "res1", "res2"):
        res = (lambda then, t=t: _with_res([t], then)) if t.startswith("res") else (lambda then: then)
        for by in (1, 2, 4, -1, -2, -4):
            p.append((f"{t}_cs{by:+d}", "all", res(_add(**{t + "_cs": by}))))
        for by in (1, 2, 4):
            p.append((f"{t}_coff{by:+d}", "all", res(_add(**{t + "_coff": by}))))
        for by in (1, 2, 4, 8):       # room in the row for the offset: only its alignment is left to object to
            p.append((f"{t}_cs+8_coff{by:+d}", "all", res(_add(**{t + "_cs": 8, t + "_coff": by}))))
    for t in ("inp", "wpk", "out", "bias", "res1", "res2"):
        for by in (4, 8):
            p.append((f"{t}_ptr+{by}", "all", _with_res(["res1", "res2"], _add(**{t: by}))))
    p += [("cout_store=cout-4", "all", lambda d: d.update(cout_store=_r(d["cout"], 4) - 4)),
          ("cout_store=32NT+4", "all", lambda d: d.update(cout_store=_r(d["cout"], 32) + 4, out_cs=_r(d["cout"], 32) + 8)),
          ("cout_store_past_out_cs", "all", lambda d: d.update(out_cs=d["cout_store"] - 4)),
          ("cout_store+1", "all", lambda d: d.update(cout_store=d["cout_store"] + 1, out_cs=d["out_cs"] + 8)),
          ("cout_store+2", "all", lambda d: d.update(cout_store=d["cout_store"] + 2, out_cs=d["out_cs"] + 8)),
          ("cout_store=32NT", "all", lambda d: d.update(cout_store=_r(d["cout"], 32), out_cs=_r(d["cout"], 32))),
          ("res1", "all", _with_res(["res1"])), ("res2", "all", _with_res(["res2"])), ("res1+res2", "all", _with_res(["res1", "res2"])),
          ("no_bias", "all", _set(bias=None))]
    for ax in "XYZ":
        p += [(f"O{ax}-1", "all", _add(**{"O" + ax: -1})), (f"o_off_{ax.lower()}+1", "all", _add(**{"o_off_" + ax.lower(): 1})),
              (f"o_stride_{ax.lower()}+1", "all", _add(**{"o_stride_" + ax.lower(): 1}))]
    for c in range(5):
        p += [(f"act_in={c}", "all", _set(act_in=c)), (f"act_out={c}", "all", _set(act_out=c))]
    p += [(f"tile_hint={h}", "all", _set(tile_hint=h)) for h in range(1, 11)]
    p += [(f"batch={b}", "all", _set(batch=b)) for b in (8191, 8192, 32767, 32768, 65535, 65536)]
    # a phase that differs from phase 0: in a field that must match (each value valid on its own) ...
    for name, f in (("inp+16", _add(inp=16)), ("out+16", _add(out=16)), ("bias+16", _add(bias=16)), ("res1", _with_res(["res1"])),
                    ("batch+1", _add(batch=1)), ("X+1", _add(X=1)), ("Y+1", _add(Y=1)), ("cin-8", _add(cin=-8)), ("cout-4", _add(cout=-4)),
                    ("in_cs+8", _add(in_cs=8)), ("out_cs+8", _add(out_cs=8)), ("px+1", _add(px=1)), ("sy+1", _add(sy=1)),
                    ("dz+1", _add(dz=1)), ("OX+1", _add(OX=1)), ("Zo-1", _add(Zo=-1)), ("act_in=1", _set(act_in=1)),
                    ("act_out=1", _set(act_out=1)), ("tile_hint=2", _set(tile_hint=2)), ("res2_cs=4", _set(res2_cs=4)),
                    # ... and in the fields that may differ
                    ("wpk+16", _add(wpk=16)), ("kx+1", _add(kx=1)), ("ky+1_kz+1", _add(ky=1, kz=1)), ("o_off_x=0", _set(o_off_x=0))):
        p.append(("phase1:" + name, "one", f))
    return p


MODES = (0, 1, 2, 3, 4, 5)       # OCCD_CONV_* and one past them
NS = (1, 2, 8, 3)                # legal phase counts and an illegal one
CALLS = (["k2", *[f"k2_phases_n{n}" for n in NS]] + [f"k2b_m{m}" for m in MODES]
         + [f"k2b_phases_m{m}_n{n}" for m in MODES for n in NS])


def _args(descs):
    arr = (hip.Conv3dArgs * MAXN)()
    for a, d in zip(arr, descs):
        for k, v in d.items():
            setattr(a, k, v)
    return arr


def codes_of(descs):
    """The return code of every entry of CALLS on the descriptors, as a string of digits (0 OK, 1 EINVAL, 2 ELAUNCH, 3 ENOMEM)."""
    lib = hip.load()
    arr = _args(descs)
    out = [lib.occd_conv3d_fwd(arr, None)] + [lib.occd_conv3d_fwd_phases(arr, n, None) for n in NS]
    out += [lib.occd_conv3d_bf16_fwd(arr, m, None) for m in MODES]
    out += [lib.occd_conv3d_bf16_fwd_phases(arr, n, m, None) for m in MODES for n in NS]
    assert all(-3 <= c <= 0 for c in out), out
    return "".join(str(-c) for c in out)


def record_codes():
    """{base: {perturbation: codes}}; needs a machine WITHOUT a device."""
    assert not torch.cuda.is_available(), "placeholder pointers must never reach a device"
    table = {}
    for base, descs in BASES.items():
        rows = {}
        for name, scope, f in perturbations():
            ds = [dict(d) for d in descs]
            for d in (ds if scope == "all" else ds[1:2]):
                f(d)
            rows[name] = codes_of(ds)
        table[base] = rows
    return table


# ------------------------------------------------------------------------------------------------- cuda: launches
def _rand(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _vox(t, C, dtype):
    return hip.Vox(t.to(dtype).cuda(), C)


PACK = {"k2": lambda w: hip.pack_weights(w), "f32": lambda w: hip.pack_weights_bf16(w), "bf16": lambda w: hip.pack_weights_bf16(w),
        "bf16x3": lambda w: hip.pack_weights_bf16(w, split3=True), "f16x2": lambda w: hip.pack_weights_f16x2(w),
        "f16x2_head": lambda w: hip.pack_weights_f16x2(w)}
FLAGS = {"f32": {}, "bf16": {}, "bf16x3": dict(split3=True), "f16x2": dict(f16x2=True)}
PLAIN = {   # name: (cin, cout, dims, in_cs, out_cs, stride, dilation, bias + both residuals + relu)
    "64_64_8x8x8_full": (64, 64, (8, 8, 8), 64, 64, 1, 1, True),
    "40_20_5x3x5": (40, 20, (5, 3, 5), 40, 24, 1, 1, False),
    "256_256_8x8x4": (256, 256, (8, 8, 4), 256, 256, 1, 1, False),
    "48_64_16x12x8_s2": (48, 64, (16, 12, 8), 48, 64, 2, 1, False),
    "64_48_16x12x8_d2": (64, 48, (16, 12, 8), 64, 48, 1, 2, False),
}
HEAD = (32, 32, (32, 128, 32), 32, 32, 1, 1, False)


def _plain(spec, kind, seed):
    cin, cout, dims, in_cs, out_cs, s, d, full = spec
    gen = torch.Generator().manual_seed(seed)
    dtype = torch.bfloat16 if kind == "bf16" else torch.float32
    pad = d                                                                    # k3 "same"
    odims = tuple((n + 2 * pad - 2 * d - 1) // s + 1 for n in dims)
    xb = torch.zeros((1,) + dims + (in_cs,))
    xb[..., :cin] = _rand(gen, 1, *dims, cin)
    x = _vox(xb, cin, dtype)
    wpk = PACK[kind]((_rand(gen, cout, cin, 3, 3, 3) / (27 * cin) ** 0.5).cuda())
    out = _vox(torch.zeros((1,) + odims + (out_cs,)), cout, dtype)
    kw = dict(stride=(s,) * 3, dilation=(d,) * 3, padding=(pad,) * 3)
    bias = None
    if full:
        bias = torch.zeros(_r(cout, 32))
        bias[:cout] = _rand(gen, cout)
        bias = bias.cuda()
        kw.update(res1=_vox(_rand(gen, 1, *odims, out_cs), cout, dtype), res2=_vox(_rand(gen, 1, *odims, out_cs), cout, dtype),
                  act_out=hip.ACT_RELU)
    if kind == "k2":
        return out, lambda: hip.conv3d(x, wpk, bias, cout, (3, 3, 3), out, **kw)
    if kind == "f16x2_head":
        return out, lambda: hip.conv3d_f16x2(x, wpk, bias, cout, (3, 3, 3), out, **kw)
    return out, lambda: hip.conv3d_bf16(x, wpk, bias, cout, (3, 3, 3), out, **kw, **FLAGS[kind])


def _phases(cin, cout, dims, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    x = _vox(_rand(gen, 1, *dims, cin), cin, torch.float32)
    out = _vox(torch.zeros((1,) + tuple(2 * n for n in dims) + (cout,)), cout, torch.float32)
    phases = []
    for px in (0, 1):
        for py in (0, 1):
            for pz in (0, 1):
                k = (1 + px, 1 + py, 1 + pz)
                phases.append((PACK[kind]((_rand(gen, cout, cin, *k) / (8 * cin) ** 0.5).cuda()), k, (px, py, pz)))
    return out, lambda: hip.conv3d_phases(x, phases, None, cout, out, act_out=hip.ACT_RELU, out_pos=dims, o_stride=(2, 2, 2),
                                          **FLAGS.get(kind, {}))


def launches():
    """{name: builder}; a builder returns (out Vox, thunk that launches once)."""
    L = {}
    for i, (name, spec) in enumerate(PLAIN.items()):
        for j, kind in enumerate(("k2", "f32", "bf16", "bf16x3", "f16x2")):
            L[f"{kind}:{name}"] = lambda spec=spec, kind=kind, seed=100 + 10 * i + j: _plain(spec, kind, seed)
    for j, kind in enumerate(("k2", "bf16x3", "f16x2")):
        L[f"{kind}:phases8_64_32_8x8x4"] = lambda kind=kind, seed=200 + j: _phases(64, 32, (8, 8, 4), kind, seed)
    L["k2:phases8_32_16_8x8x4"] = lambda: _phases(32, 16, (8, 8, 4), "k2", 210)
    for j, kind in enumerate(("k2", "bf16x3", "f16x2_head")):
        L[f"{kind}:head_32_32_32x128x32"] = lambda kind=kind, seed=300 + j: _plain(HEAD, kind, seed)
    return L


def record_launches():
    """{name: {"rows": {tag: [launches, flops, bytes]}, "sha256": of the output buffer's bytes}}."""
    table = {}
    for name, build in launches().items():
        out, run = build()
        torch.cuda.synchronize()
        with hip.profile() as prof:
            run()
            torch.cuda.synchronize()
        raw = out.buf.view(torch.int16 if out.buf.dtype == torch.bfloat16 else torch.int32).cpu().numpy().tobytes()
        table[name] = dict(rows={tag: [r["launches"], r["flops"], r["bytes"]] for tag, r in sorted(prof.rows.items())},
                           sha256=hashlib.sha256(raw).hexdigest())
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", choices=("cpu", "cuda"), required=True)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.device == "cpu" and torch.cuda.is_available():
        sys.exit("the return codes are recorded on a machine without a device (placeholder pointers)")
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    if a.device == "cpu":
        doc["calls"], doc["codes"] = CALLS, record_codes()
        n = sum(len(v) for v in doc["codes"].values())
        print(f"cpu: {len(doc['codes'])} bases, {n} descriptors x {len(CALLS)} calls -> {a.out}")
    else:
        doc["launches"] = record_launches()
        print(f"cuda: {len(doc['launches'])} launches -> {a.out}")
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
