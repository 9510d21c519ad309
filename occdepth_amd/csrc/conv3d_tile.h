// What the implicit-GEMM 3-D convolutions K2 (conv3d_igemm.hip, fp32 matrix pipe) and K2b (conv3d_bf16.hip, bf16 / f16 pipe)
// share: one GEMM view (M = output voxels in TY x TZ tiles of one x plane, N = Cout, K = taps x Cin), one output scatter, one
// launch descriptor.  Host side: validation, the phase-consistency check, the fill of the kernel parameters and the launch
// tail.  Device side: the source index of the weight packers.  Each file keeps its parameter structs (their offsets are the
// kernarg offsets; the field names agree, so the templates below fill either), its variant table, its tiling plan and variant
// choice, and its whole kernel.  The kernels' twin passages -- tile decode, M-row decode, split-K reduction through LDS,
// output-voxel index -- are NOT here: as __forceinline__ functions (by reference to the parameter struct or with scalar
// arguments alike) each of them changed the register allocation and instruction order of both files' code objects, and
// this project changes a kernel's machine code on purpose and with a measurement, or not at all.
#pragma once
#include "device.h"

#include <algorithm>
#include <cstddef>
#include <cstring>

namespace occd {

constexpr int kMaxPhases = 8;
constexpr size_t kMaxConvLds = 160 * 1024;

// ---------------------------------------------------------------------------------------------------------------- host
// How a kernel stores its activation tensors (in / out / res1 / res2; bias is float32 and the weights 16-byte records for all).
struct ConvStorage {
    int esz;            // bytes per element
    int align;          // staging loads are 16 bytes: in_cs / in_coff are multiples of `align` elements
    unsigned act_in;    // bit c set: act_in code c is accepted (kAnyActIn: the code is not looked at)
};
constexpr unsigned kAnyActIn = ~0u;

inline bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }

inline int conv3d_validate(const occd_conv3d_args* a, const ConvStorage& st) {
    if (!a || !a->in || !a->wpk || !a->out) return OCCD_EINVAL;
    if (a->batch <= 0 || a->X <= 0 || a->Y <= 0 || a->Z <= 0 || a->cin <= 0 || a->cout <= 0) return OCCD_EINVAL;
    if (a->kx <= 0 || a->ky <= 0 || a->kz <= 0 || a->sx <= 0 || a->sy <= 0 || a->sz <= 0) return OCCD_EINVAL;
    if (a->Xo <= 0 || a->Yo <= 0 || a->Zo <= 0) return OCCD_EINVAL;
    const int cin8 = (a->cin + 7) & ~7;
    const int NTtot = (a->cout + 31) / 32;
    // every staged 16-byte load must be aligned and inside the row
    if ((a->in_cs & (st.align - 1)) || (a->in_coff & (st.align - 1)) || a->in_coff + cin8 > a->in_cs) return OCCD_EINVAL;
    if (misaligned(a->in, 16) || misaligned(a->wpk, 16)) return OCCD_EINVAL;
    if (a->cout_store < a->cout || a->cout_store > NTtot * 32 || a->out_coff + a->cout_store > a->out_cs)
        return OCCD_EINVAL;
    // 4-channel epilogue groups (16 B float32 / 8 B bf16 accesses): rows, slices and the stored width are multiples of 4
    const uintptr_t grp = 4 * st.esz;
    if ((a->cout_store & 3) || (a->out_cs & 3) || (a->out_coff & 3) || misaligned(a->out, grp)) return OCCD_EINVAL;
    if (a->res1 && ((a->res1_cs & 3) || (a->res1_coff & 3) || misaligned(a->res1, grp) ||
                    a->res1_coff + a->cout_store > a->res1_cs))
        return OCCD_EINVAL;
    if (a->res2 && ((a->res2_cs & 3) || (a->res2_coff & 3) || misaligned(a->res2, grp) ||
                    a->res2_coff + a->cout_store > a->res2_cs))
        return OCCD_EINVAL;
    if (a->bias && misaligned(a->bias, 16)) return OCCD_EINVAL;
    if ((a->Xo - 1) * a->o_stride_x + a->o_off_x >= a->OX || (a->Yo - 1) * a->o_stride_y + a->o_off_y >= a->OY ||
        (a->Zo - 1) * a->o_stride_z + a->o_off_z >= a->OZ)
        return OCCD_EINVAL;
    if (st.act_in != kAnyActIn && ((unsigned)a->act_in >= 32u || !(st.act_in >> a->act_in & 1u))) return OCCD_EINVAL;
    if (a->act_out != OCCD_ACT_NONE && a->act_out != OCCD_ACT_RELU && a->act_out != OCCD_ACT_RELU_PRE)
        return OCCD_EINVAL;
    return OCCD_OK;
}

// The sub-pixel phases a[0..n) of ONE transposed convolution, n in {1, 2, 4, 8}: each valid, and they differ ONLY in wpk,
// kx / ky / kz and o_off_*.
inline int conv3d_validate_phases(const occd_conv3d_args* a, int n, const ConvStorage& st) {
    if (!a || (n != 1 && n != 2 && n != 4 && n != 8)) return OCCD_EINVAL;
    for (int i = 0; i < n; ++i) {
        const int bad = conv3d_validate(a + i, st);
        if (bad != OCCD_OK) return bad;
        occd_conv3d_args t = a[i];
        t.wpk = a[0].wpk; t.kx = a[0].kx; t.ky = a[0].ky; t.kz = a[0].kz;
        t.o_off_x = a[0].o_off_x; t.o_off_y = a[0].o_off_y; t.o_off_z = a[0].o_off_z;
        if (memcmp(&t, &a[0], offsetof(occd_conv3d_args, tile_hint) + sizeof(int32_t)) != 0) return OCCD_EINVAL;
    }
    return OCCD_OK;
}

// One variant and one output tiling serve all phases of a launch: plan for a[0] with the largest ky / kz over the phases
// (the largest slab), with batch x n copies of the tile grid.
inline occd_conv3d_args conv3d_widest_phase(const occd_conv3d_args* a, int n) {
    occd_conv3d_args big = a[0];
    for (int i = 1; i < n; ++i) {
        big.ky = std::max(big.ky, a[i].ky);
        big.kz = std::max(big.kz, a[i].kz);
    }
    return big;
}

// A TY x TZ tile of output voxels per workgroup, the slab YIN x ZIN it stages, and the grid that follows (plan() / plan_b()).
struct Tiling {
    int TY, TZ, YIN, ZIN, ytiles, ztiles, ngroups;
    size_t lds;
    long nwg;
    double cost;    // plan_b's ranking of its candidates
};

// What the caller chose: the tail below neither picks a variant nor knows a kernel's template parameters.
struct ConvLaunch {
    const char* name;      // profile row
    int block;             // threads per workgroup
    size_t row_bytes;      // LDS bytes per staged slab row, over all K groups
    ConvStorage st;
    double wbytes;         // bytes per weight element streamed (the cost model of the profile row)
    bool any_batch;        // occd_conv3d_fwd alone leaves batch > 65535 (the grid's y limit) to the runtime, as it always has
};

// Geometry -> the fields every parameter struct has under the same names.  KTtot (K2), cin16 / K16tot and PhaseBP::fac (K2b)
// and the weight pointers (typed per kernel) stay with their file.
template <class P>
void conv3d_fill(const occd_conv3d_args* a, const Tiling& til, P* p) {
    p->in = a->in; p->bias = a->bias; p->res1 = a->res1; p->res2 = a->res2; p->out = a->out;
    p->X = a->X; p->Y = a->Y; p->Z = a->Z; p->cin8 = (a->cin + 7) & ~7; p->in_cs = a->in_cs; p->in_coff = a->in_coff;
    p->NTtot = (a->cout + 31) / 32;
    p->out_cs = a->out_cs; p->out_coff = a->out_coff;
    p->res1_cs = a->res1_cs; p->res1_coff = a->res1_coff; p->res2_cs = a->res2_cs; p->res2_coff = a->res2_coff;
    p->SX = a->sx; p->SY = a->sy; p->SZ = a->sz;
    p->DX = a->dx; p->DY = a->dy; p->DZ = a->dz; p->PX = a->px; p->PY = a->py; p->PZ = a->pz;
    p->Xo = a->Xo; p->Yo = a->Yo; p->Zo = a->Zo; p->OX = a->OX; p->OY = a->OY; p->OZ = a->OZ;
    p->osx = a->o_stride_x; p->osy = a->o_stride_y; p->osz = a->o_stride_z;
    p->act_in = a->act_in; p->act_out = a->act_out; p->cout_store = a->cout_store;
    p->TY = til.TY; p->TZ = til.TZ;
    p->ytiles = til.ytiles; p->ztiles = til.ztiles; p->nwg = (int)til.nwg;
    p->div_tz = make_fastdiv(til.TZ);
    p->div_ztiles = make_fastdiv(til.ztiles); p->div_ytiles = make_fastdiv(til.ytiles);
}

template <class PH>
void conv3d_fill_phase(const occd_conv3d_args* a, const Tiling& til, PH* ph) {
    ph->KX = a->kx; ph->KY = a->ky; ph->KZ = a->kz;
    ph->oox = a->o_off_x; ph->ooy = a->o_off_y; ph->ooz = a->o_off_z;
    ph->YIN = (til.TY - 1) * a->sy + (a->ky - 1) * a->dy + 1;      // (the shared tile, this phase's extent)
    ph->ZIN = (til.TZ - 1) * a->sz + (a->kz - 1) * a->dz + 1;
    ph->div_zin = make_fastdiv(ph->ZIN);
}

// Phase-major dispatch (all tiles of the heaviest phase first) is the default; the phases of a tile next to each other on one
// XCD (the switch below set to 1) measured SLOWER: 64 -> 32 at 128x128x16 0.47 against 0.35 ms on K2, 0.36 against 0.34 on K2b.
inline bool conv3d_phase_fast() {
    static const bool on = env_flag("OCCD_PHASE_FAST", false);
    return on;
}

// The launch of n phases (n = 1: a plain convolution) as ONE grid: the phase is the low bits of blockIdx.y, every phase walks
// the same output tiling of the (shared) input volume, and the heaviest tap subset comes first in dispatch order so that the
// single-tap phases fill the tail.  `p` arrives with the caller's own fields set; set_weights(p.ph[i], phase) sets the typed
// weight pointers of a phase.
template <class P, class SetWeights>
int conv3d_launch(const occd_conv3d_args* a, int n, const Tiling& til, void (*kern)(const P), P& p, const ConvLaunch& L,
                  SetWeights set_weights, hipStream_t stream) {
    const long copies = (long)a->batch * n;
    if ((copies > 65535 && !L.any_batch) || til.nwg * n >= (1L << 24)) return OCCD_EINVAL;
    conv3d_fill(a, til, &p);
    p.nph_log2 = n == 1 ? 0 : n == 2 ? 1 : n == 4 ? 2 : 3;
    p.ph_fast = n > 1 && conv3d_phase_fast() ? 1 : 0;
    if (p.ph_fast) p.nwg = (int)(til.nwg * n);
    int order[kMaxPhases];
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order, order + n, [&](int l, int r) { return a[l].kx * a[l].ky * a[l].kz > a[r].kx * a[r].ky * a[r].kz; });
    double flops = 0.0, bytes = 0.0;
    const double pos = (double)a->batch * a->Xo * a->Yo * a->Zo;
    for (int i = 0; i < n; ++i) {
        const occd_conv3d_args* ai = a + order[i];
        conv3d_fill_phase(ai, til, &p.ph[i]);
        set_weights(p.ph[i], *ai);
        if ((size_t)p.ph[i].YIN * p.ph[i].ZIN * L.row_bytes > til.lds) return OCCD_EINVAL;
        const double taps = (double)ai->kx * ai->ky * ai->kz;
        flops += 2.0 * pos * taps * ai->cin * ai->cout;
        bytes += (double)L.st.esz * ((i == 0 ? (double)a->batch * a->X * a->Y * a->Z * a->cin : 0.0) +
                                     pos * a->cout * (1 + (a->res1 != nullptr) + (a->res2 != nullptr))) +
                 L.wbytes * taps * a->cin * a->cout;
    }
    if (til.lds > 64 * 1024 && ensure_big_lds(reinterpret_cast<const void*>(kern)) != OCCD_OK) return OCCD_ELAUNCH;
    ProfScope prof(L.name, stream, flops, bytes);
    hipLaunchKernelGGL(kern, p.ph_fast ? dim3((unsigned)(til.nwg * n), (unsigned)a->batch, (unsigned)til.ngroups)
                                       : dim3((unsigned)til.nwg, (unsigned)copies, (unsigned)til.ngroups),
                       dim3(L.block), til.lds, stream, p);
    return check_launch();
}

}  // namespace occd

// -------------------------------------------------------------------------------------------------------------- device
// Element (co, ci, tap) of the operator a weight packer reads.  layout 0: w[co][ci][tap]; 1: w[ci][co][tap] (transposed
// convolution weights); 2: w[ci][co], a row-major GEMM B operand; 3 (`tm` given, the *_gather entry points):
// w[co * s_co + ci * s_ci + ofs[tap]] -- any transposed / flipped / tap-subset view of a dense weight tensor without
// materialising it (the data-gradient phases).
__device__ __forceinline__ float conv3d_weight_src(const float* __restrict__ w, int layout, int co, int ci, int tap, int cout,
                                                   int cin, int taps, const occd::TapMap* tm) {
    if (layout == 0) return w[((size_t)co * cin + ci) * taps + tap];
    if (layout == 1) return w[((size_t)ci * cout + co) * taps + tap];
    if (tm == nullptr || layout == 2) return w[(size_t)ci * cout + co];
    return w[(size_t)co * tm->s_co + (size_t)ci * tm->s_ci + tm->ofs[tap]];
}
