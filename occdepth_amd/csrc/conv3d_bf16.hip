// K2b -- implicit-GEMM 3-D convolution on the CDNA4 bf16 matrix pipe (BASELINE configs[3]: the bf16 training step).
//
//   out[vox][co] = act_out( sum_{tap,ci} bf16(act_in(in[vox*stride - pad + tap*dil][ci])) * bf16(W[co][ci][tap])
//                           + bias[co] + res1[vox][co] + res2[vox][co] )          (fp32 accumulate)
//
// Same GEMM view, tiling, output scatter and epilogue as K2 (conv3d_igemm.hip), same validation, parameter fill and launch
// (conv3d_tile.h); what changes is the instruction --
// v_mfma_f32_32x32x16_bf16: 16 K values per instruction at 32 cycles, 16x the fp32 MFMA rate -- and with it the
// bottleneck: operand delivery.  A wave therefore owns up to 4 x 2 tiles of 32 voxels x 32 couts (each B fragment
// loaded from L2 feeds MT MFMAs, each A fragment read from LDS feeds NT), the staged slab holds bf16 (half the LDS
// bytes: [YIN][ZIN][32 channels] rows of 64 B + 16 B pad, an odd number of 16-B slots -> conflict-free ds_read_b128),
// and activations may live in HBM as fp32 (converted once, while staging: "bf16 MFMA, fp32 storage") or as bf16.
// Fragment layout (pinned on hardware by tools/probe_bf16.hip): lane l holds 8 consecutive K values 8 (l >> 5) + j of
// row / column l & 31; D as for every 32x32 MFMA: column = l & 31, row = (r & 3) + 8 (r >> 2) + 4 (l >> 5).
// The 2-D decoder's 3x3 convolutions run through the same kernel as X = 1 volumes of channels-last (NHWC) images.
//
// Reference semantics replaced (training step, N1): occdepth/models/DDR.py:111-139, modules.py:40-46,158-175,278-296,
// CRP3D.py:54-97, unet2d.py:24-46 -- forward and, on dL/dy with flipped weights, the data gradient.
#include "conv3d_tile.h"

using occd::FastDiv;
using occd::Tiling;

namespace {

// what differs between the sub-pixel phases of one transposed convolution (see K2's PhaseP, csrc/conv3d_igemm.hip)
struct PhaseBP {
    const u32x4* wpk;
    const float* fac;       // SPLIT = 2: the per-cout epilogue factors of this phase's image (its trailer)
    int KX, KY, KZ, oox, ooy, ooz, YIN, ZIN;
    FastDiv div_zin;
};

struct ConvBP {
    const void* in;
    const float* bias;
    const void* res1;
    const void* res2;
    void* out;
    int X, Y, Z, cin8, cin16, in_cs, in_coff;
    int K16tot, NTtot;
    int out_cs, out_coff, res1_cs, res1_coff, res2_cs, res2_coff;
    int SX, SY, SZ, DX, DY, DZ, PX, PY, PZ;
    int Xo, Yo, Zo, OX, OY, OZ, osx, osy, osz;
    int act_in, act_out, cout_store;
    int TY, TZ, ytiles, ztiles, nwg;
    int nph_log2;           // blockIdx.y = (batch index << nph_log2) | phase, or (ph_fast) linear id = (tile << nph_log2) | phase
    int ph_fast;
    FastDiv div_tz, div_ztiles, div_ytiles;
    PhaseBP ph[occd::kMaxPhases];
};

__device__ __forceinline__ f32x4 unpack_lo(u32x2 v) {       // 4 bf16 -> 4 floats
    f32x4 r;
    r.x = __builtin_bit_cast(float, v.x << 16);
    r.y = __builtin_bit_cast(float, v.x & 0xffff0000u);
    r.z = __builtin_bit_cast(float, v.y << 16);
    r.w = __builtin_bit_cast(float, v.y & 0xffff0000u);
    return r;
}

constexpr int kRSB = 80;   // LDS row stride in bytes: 32 bf16 channels + 16 B pad
constexpr int kRSB3 = 208; // SPLIT = 3: three bf16 planes (hi, mid, lo) of the 32 channels + 16 B pad (13 slots: odd)
constexpr int kRSB2 = 144; // SPLIT = 2: two fp16 planes (hi, lo') of the 32 channels + 16 B pad (9 slots: odd)

// (activations act3d_x4, pack_bf16x8 and the three-term split split3_bf16x8: device.h)

// SPLIT = 1: plain bf16 operands.  SPLIT = 3 (opt-in experiment): float32 activations and weights as
// three bf16 terms each, six MFMAs per K step instead of one -- float32-level accuracy at 6/16 of the fp32-MFMA time.
// SPLIT = 2 (K2bh): K2s3h's numerics (csrc/conv3d_c32p.hip, design A) on this skeleton -- float32 activations staged once as
// x' = 2^kF2XExp x = hi + 2^-11 lo' (split2_f16x8), weights from the image of occd_pack_weights_f16x2 (this kernel's fragment
// order; hi | hs | lo | per-cout factors), three v_mfma_f32_32x32x16_f16 per K step: lo_w hi_x + hs_w lo'_x + hi_w hi_x, smallest
// first.  Only hi and lo stream from L2 (4 bytes per weight element instead of the 6 of SPLIT = 3, which is what bounds the
// small-volume launches); hs = hi 2^-11 is formed in registers (four v_pk_mul_f16 per fragment, fp16 denormals on: exact
// wherever the stored hs is).  The epilogue multiplies by the per-cout factor before the bias -- after the K groups are summed.
// KS > 1: in-workgroup split-K as in K2 (conv3d_igemm.hip): the KS wave groups take interleaved 32-channel chunks, each with
// its own LDS slab, and their accumulators are summed through LDS before the epilogue -- the 3x3x3 convolutions of the 1/8
// level (4096 voxels, K = 27 x 256): 128 output tiles for 256 CUs.
template <int MT, int NT, int WM, int WN, bool IN_BF16, bool OUT_BF16, int SPLIT = 1, int KS = 1>
__global__ void __launch_bounds__(WM* WN * KS * 64) conv3d_bf16_kernel(const ConvBP p) {
    constexpr int NTH = WM * WN * 64;   // threads of one K group
    constexpr int RSB = SPLIT == 3 ? kRSB3 : SPLIT == 2 ? kRSB2 : kRSB;
    constexpr int WIMG = SPLIT == 2 ? 2 : 1;   // streamed weight image sp lies WIMG * sp images into the buffer (SPLIT = 2: hi, lo)
    static_assert(SPLIT == 1 || ((SPLIT == 2 || SPLIT == 3) && !IN_BF16 && !OUT_BF16), "the splits take and return float32");
    extern __shared__ __attribute__((aligned(16))) unsigned char slab_all[];

    const int lane = threadIdx.x & 63;
    const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kg = KS == 1 ? 0 : wave_all / (WM * WN);          // K group of this wave
    const int wave = wave_all - kg * (WM * WN);
    const int tid = threadIdx.x - kg * NTH;                      // thread index inside the K group
    const int wm = wave / WN;
    const int wn = wave - wm * WN;
    const int li = lane & 31;
    const int h = lane >> 5;

    uint32_t bid = xcd_remap(blockIdx.x, p.nwg);   // an XCD walks a contiguous run of tiles
    // phase of a merged transposed-convolution launch: the low bits of the (remapped) linear id when ph_fast -- the phases of
    // one output tile run next to each other on one XCD, so their interleaved voxel rows meet in its L2 and the input tile is
    // fetched once -- else the low bits of blockIdx.y (phase-major dispatch, heaviest tap subset first)
    const uint32_t ph_mask = (1u << p.nph_log2) - 1u;
    const uint32_t ph_i = p.ph_fast ? bid & ph_mask : blockIdx.y & ph_mask;
    if (p.ph_fast) bid >>= p.nph_log2;
    const uint32_t t1 = occd_fastdiv(bid, p.div_ztiles);
    const int zt = bid - t1 * p.ztiles;
    const uint32_t t2 = occd_fastdiv(t1, p.div_ytiles);
    const int yt = t1 - t2 * p.ytiles;
    const int xo = t2;
    const int b = p.ph_fast ? blockIdx.y : blockIdx.y >> p.nph_log2;
    const PhaseBP& ph = p.ph[ph_i];
    const int nt0 = (blockIdx.z * WN + wn) * NT;

    int rowbase[MT];   // byte offset of this lane's A row (tap (0,0), k16 0) for each M tile
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const uint32_t m = (wm * MT + mt) * 32 + li;
        uint32_t yl = occd_fastdiv(m, p.div_tz);
        uint32_t zl = m - yl * p.TZ;
        const bool in_tile = yl < (uint32_t)p.TY;
        yl = in_tile ? yl : 0u;
        zl = in_tile ? zl : 0u;
        rowbase[mt] = (int)((yl * p.SY) * ph.ZIN + zl * p.SZ) * RSB + h * 16;
    }
    int wofs[NT];      // u32x4 index of each owned N tile inside one (tap, k16) weight record row
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wofs[nt] = min(nt0 + nt, p.NTtot - 1) * 64;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    const int y_in0 = yt * p.TY * p.SY - p.PY;
    const int z_in0 = zt * p.TZ * p.SZ - p.PZ;
    const size_t w_step = (size_t)p.NTtot * 64;          // u32x4 per (tap, k16)
    const size_t w_img = (size_t)ph.KX * ph.KY * ph.KZ * p.K16tot * w_step;   // u32x4 per split image of the weights
    const u32x4* const wlane = ph.wpk + lane;
    const int rows = ph.YIN * ph.ZIN;
    unsigned char* const slab = slab_all + (size_t)kg * rows * RSB;   // this K group's slab
    const int n_chunks = (p.cin16 + 31) / 32;
    const int chunk_iters = (n_chunks + KS - 1) / KS;

#define OCCD_MFMA1(WS, XS)                                                                                          \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, b_cur[nt][WS]),                         \
                                                __builtin_bit_cast(bf16x8, a_cur[mt][XS]), acc[mt][nt], 0, 0, 0)
#define OCCD_MFMA1H(W, XS)                                                                                          \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = \
        __builtin_amdgcn_mfma_f32_32x32x16_f16(W, __builtin_bit_cast(f16x8, a_cur[mt][XS]), acc[mt][nt], 0, 0, 0)
    // smallest terms first: (mid, mid), (hi, lo), (lo, hi), (hi, mid), (mid, hi), (hi, hi); SPLIT = 2: (lo, hi), (hs, lo'), (hi, hi)
#define OCCD_MFMA_BLOCK()                                                  \
    if (SPLIT == 2) {                                                      \
        f16x8 w_hs[NT];                                                    \
        _Pragma("unroll") for (int nt = 0; nt < NT; ++nt)                  \
            w_hs[nt] = __builtin_bit_cast(f16x8, b_cur[nt][0]) * (_Float16)(1.f / 2048.f); \
        OCCD_MFMA1H(__builtin_bit_cast(f16x8, b_cur[nt][SPLIT == 2 ? 1 : 0]), 0); \
        OCCD_MFMA1H(w_hs[nt], SPLIT == 2 ? 1 : 0);                         \
        OCCD_MFMA1H(__builtin_bit_cast(f16x8, b_cur[nt][0]), 0);           \
    } else if (SPLIT == 3) {                                               \
        OCCD_MFMA1(SPLIT == 3 ? 1 : 0, SPLIT == 3 ? 1 : 0);                \
        OCCD_MFMA1(0, SPLIT == 3 ? 2 : 0);                                 \
        OCCD_MFMA1(SPLIT == 3 ? 2 : 0, 0);                                 \
        OCCD_MFMA1(0, SPLIT == 3 ? 1 : 0);                                 \
        OCCD_MFMA1(SPLIT == 3 ? 1 : 0, 0);                                 \
    }                                                                      \
    if (SPLIT != 2) { OCCD_MFMA1(0, 0); }

    for (int kx = 0; kx < ph.KX; ++kx) {
        const int xi = xo * p.SX - p.PX + kx * p.DX;
        if (xi < 0 || xi >= p.X) continue;   // workgroup-uniform
        const size_t plane = ((size_t)(b * p.X + xi) * p.Y) * p.Z * p.in_cs + p.in_coff;
        for (int ci = 0; ci < chunk_iters; ++ci) {
            const int c0 = (ci * KS + kg) * 32;
            const bool active = KS == 1 || c0 < p.cin16;     // uniform per K group; every group still joins the barriers
            const int ck = active ? min(32, p.cin16 - c0) : 16;   // 16 or 32 channels in this chunk
            const int k16n = ck >> 4;
            const int sh = k16n;                         // chunks of 8 channels per row: 2 (shift 1) or 4 (shift 2)
            const int S = active ? ph.KY * ph.KZ * k16n : 0;
            const u32x4* wp = wlane + ((size_t)(kx * ph.KY * ph.KZ) * p.K16tot + (active ? c0 >> 4 : 0)) * w_step;

            u32x4 b_cur[NT][SPLIT];   // first B fragments fly while the slab is staged
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int sp = 0; sp < SPLIT; ++sp) b_cur[nt][sp] = wp[wofs[nt] + sp * WIMG * w_img];

            __syncthreads();   // previous slab fully consumed
            const int F = rows << sh;
            for (int f0 = 0; active && f0 < F; f0 += NTH * 4) {
                u32x4 v[4][SPLIT];
                int dst[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int f = f0 + u * NTH + tid;
                    const int fc = min(f, F - 1);
                    const uint32_t row = (uint32_t)fc >> sh;
                    const int c8 = fc & ((1 << sh) - 1);
                    const uint32_t yi = occd_fastdiv(row, ph.div_zin);
                    const int zi = (int)row - (int)yi * ph.ZIN;
                    const int y = y_in0 + (int)yi, z = z_in0 + zi;
                    const int c = c0 + c8 * 8;
                    const bool ok = f < F && c < p.cin8 && (unsigned)y < (unsigned)p.Y && (unsigned)z < (unsigned)p.Z;
                    const int yc = min(max(y, 0), p.Y - 1), zc = min(max(z, 0), p.Z - 1);
                    const int cc = min(c, p.cin8 - 8);
                    const size_t e = plane + ((size_t)yc * p.Z + zc) * p.in_cs + cc;
                    u32x4 w[SPLIT];
                    if (IN_BF16) {
                        w[0] = *(const u32x4*)((const uint16_t*)p.in + e);
                        if (p.act_in == OCCD_ACT_RELU) {   // bf16 relu on the packed pairs: clear negative halves
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                uint32_t d = w[0][q];
                                if (d & 0x80000000u) d &= 0x0000ffffu;
                                if (d & 0x00008000u) d &= 0xffff0000u;
                                w[0][q] = d;
                            }
                        }
                    } else {
                        f32x4 lo = *(const f32x4*)((const float*)p.in + e);
                        f32x4 hi = *(const f32x4*)((const float*)p.in + e + 4);
                        if (p.act_in == OCCD_ACT_RELU) { lo = act3d_x4(lo, OCCD_ACT_RELU); hi = act3d_x4(hi, OCCD_ACT_RELU); }
                        else if (SPLIT == 3 && p.act_in == OCCD_ACT_SIGMOID) {
                            lo = act3d_x4(lo, OCCD_ACT_SIGMOID); hi = act3d_x4(hi, OCCD_ACT_SIGMOID);
                        }
                        if (SPLIT == 3) split3_bf16x8(lo, hi, w[0], w[SPLIT == 3 ? 1 : 0], w[SPLIT == 3 ? 2 : 0]);
                        else if (SPLIT == 2) split2_f16x8(lo, hi, w[0], w[SPLIT == 2 ? 1 : 0]);
                        else w[0] = pack_bf16x8(lo, hi);
                    }
#pragma unroll
                    for (int sp = 0; sp < SPLIT; ++sp) v[u][sp] = ok ? w[sp] : u32x4{0u, 0u, 0u, 0u};
                    dst[u] = f < F ? (int)row * RSB + c8 * 16 : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (dst[u] >= 0) {
#pragma unroll
                        for (int sp = 0; sp < SPLIT; ++sp) *(u32x4*)(slab + dst[u] + sp * 64) = v[u][sp];
                    }
            }
            __syncthreads();

            int ky = 0, kz = 0, kl = 0;
            int lds_off = 0;   // bytes
            u32x4 a_cur[MT][SPLIT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int sp = 0; sp < SPLIT; ++sp) a_cur[mt][sp] = *(const u32x4*)(slab + rowbase[mt] + sp * 64);

            for (int s = 0; s < S - 1; ++s) {
                ++kl;
                lds_off += 32;
                wp += w_step;
                if (kl == k16n) {
                    kl = 0;
                    wp += (size_t)(p.K16tot - k16n) * w_step;
                    if (++kz == ph.KZ) { kz = 0; ++ky; }
                    lds_off = (ky * p.DY * ph.ZIN + kz * p.DZ) * RSB;
                }
                u32x4 a_nxt[MT][SPLIT], b_nxt[NT][SPLIT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int sp = 0; sp < SPLIT; ++sp) a_nxt[mt][sp] = *(const u32x4*)(slab + rowbase[mt] + lds_off + sp * 64);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int sp = 0; sp < SPLIT; ++sp) b_nxt[nt][sp] = wp[wofs[nt] + sp * WIMG * w_img];
                OCCD_MFMA_BLOCK();
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int sp = 0; sp < SPLIT; ++sp) a_cur[mt][sp] = a_nxt[mt][sp];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int sp = 0; sp < SPLIT; ++sp) b_cur[nt][sp] = b_nxt[nt][sp];
            }
            if (active) { OCCD_MFMA_BLOCK(); }
        }
    }
#undef OCCD_MFMA1
#undef OCCD_MFMA1H
#undef OCCD_MFMA_BLOCK

    if (KS > 1) {
        // sum the K groups' accumulators through LDS (slabs are dead after the barrier), group 0 stores
        float* red = reinterpret_cast<float*>(slab_all);
        __syncthreads();
        if (kg > 0) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        red[((((kg - 1) * WM * WN + wave) * MT + mt) * NT + nt) * 1024 + r * 64 + lane] = acc[mt][nt][r];
        }
        __syncthreads();
        if (kg > 0) return;
#pragma unroll
        for (int g = 1; g < KS; ++g)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        acc[mt][nt][r] += red[((((g - 1) * WM * WN + wave) * MT + mt) * NT + nt) * 1024 + r * 64 + lane];
    }

    // ---------------- epilogue (the layout of K2's: lane -> voxel li of the M tile, registers -> couts
    // (r & 3) + 8 (r >> 2) + 4 h: four groups of 4 consecutive output channels of ONE voxel per lane)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const uint32_t m = (wm * MT + mt) * 32 + li;
        const uint32_t yl = occd_fastdiv(m, p.div_tz);
        const uint32_t zl = m - yl * p.TZ;
        const int yo = yt * p.TY + (int)yl, zo = zt * p.TZ + (int)zl;
        const bool ok = yl < (uint32_t)p.TY && yo < p.Yo && zo < p.Zo;
        const size_t vox = ((size_t)(b * p.OX + xo * p.osx + ph.oox) * p.OY + (yo * p.osy + ph.ooy)) * p.OZ +
                           (zo * p.osz + ph.ooz);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = (nt0 + nt) * 32 + 8 * g + 4 * h;
                if (ok && c < p.cout_store) {
                    f32x4 v = {acc[mt][nt][4 * g], acc[mt][nt][4 * g + 1], acc[mt][nt][4 * g + 2],
                               acc[mt][nt][4 * g + 3]};
                    if (SPLIT == 2) v *= *(const f32x4*)(ph.fac + c);     // 2^-(k[cout] + kF2XExp): exact
                    if (p.bias != nullptr) v += *(const f32x4*)(p.bias + c);
                    if (p.act_out == OCCD_ACT_RELU_PRE) v = act3d_x4(v, OCCD_ACT_RELU);
                    if (OUT_BF16) {
                        if (p.res1 != nullptr)
                            v += unpack_lo(*(const u32x2*)((const uint16_t*)p.res1 + vox * p.res1_cs + p.res1_coff + c));
                        if (p.res2 != nullptr)
                            v += unpack_lo(*(const u32x2*)((const uint16_t*)p.res2 + vox * p.res2_cs + p.res2_coff + c));
                    } else {
                        if (p.res1 != nullptr) v += *(const f32x4*)((const float*)p.res1 + vox * p.res1_cs + p.res1_coff + c);
                        if (p.res2 != nullptr) v += *(const f32x4*)((const float*)p.res2 + vox * p.res2_cs + p.res2_coff + c);
                    }
                    if (p.act_out == OCCD_ACT_RELU) v = act3d_x4(v, OCCD_ACT_RELU);
                    if (OUT_BF16) {
                        bf16x4 o = {(__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w};
                        *(u32x2*)((uint16_t*)p.out + vox * p.out_cs + p.out_coff + c) = __builtin_bit_cast(u32x2, o);
                    } else {
                        *(f32x4*)((float*)p.out + vox * p.out_cs + p.out_coff + c) = v;
                    }
                }
            }
        }
    }
}

// ---------------------------------------------------------------- weight packing (fp32 master weights -> bf16 fragments)
// wpk[tap][k16][nt][lane][j]: cout = nt * 32 + (lane & 31), cin = k16 * 16 + (lane >> 5) * 8 + j
// nsplit = 3: three consecutive images hi | mid | lo of the float32 weight (see split3_bf16x8, device.h)
__global__ void pack_weights_bf16_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                         uint16_t* __restrict__ wpk, int cout, int cin, int taps, int K16, int NT,
                                         int layout, long total, int nsplit, const occd::TapMap tm) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = i & 7;
    const int lane = (i >> 3) & 63;
    long t = i >> 9;
    const int nt = t % NT; t /= NT;
    const int k16 = t % K16; t /= K16;
    const int tap = (int)t;
    const int co = nt * 32 + (lane & 31);
    const int ci = k16 * 16 + (lane >> 5) * 8 + j;
    float v = 0.f;
    if (co < cout && ci < cin) {
        v = conv3d_weight_src(w, layout, co, ci, tap, cout, cin, taps, &tm);
        if (scale != nullptr) v *= scale[co];
    }
    const __bf16 hi = (__bf16)v;
    wpk[i] = __builtin_bit_cast(uint16_t, hi);
    if (nsplit == 3) {
        const float r = v - (float)hi;
        const __bf16 mid = (__bf16)r;
        wpk[i + total] = __builtin_bit_cast(uint16_t, mid);
        wpk[i + 2 * total] = __builtin_bit_cast(uint16_t, (__bf16)(r - (float)mid));
    }
}

// K2s3h weight image (occd_pack_weights_f16x2): three fp16 images in the layout above -- hi | hs | lo of w' = 2^k[co] w,
// hi = fp16(w'), hs = hi 2^-11, lo = fp16(w' - hi) -- followed by NT * 32 floats 2^-(k[co] + kF2XExp) (the epilogue factor;
// kF2XExp: the activation pre-scale of split2_f16x8, device.h).  k[co] puts max_{ci, tap} |w'| into [2^13, 2^14).
__global__ void f16x2_scale_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ fac,
                                   int cout, int cin, int taps, int NT, int layout) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= NT * 32) return;
    float m = 0.f;
    if (co < cout) {
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < taps; ++tap) {
                float v = conv3d_weight_src(w, layout, co, ci, tap, cout, cin, taps, nullptr);
                if (scale != nullptr) v *= scale[co];
                m = fmaxf(m, fabsf(v));
            }
    }
    int e = 0;
    if (m > 0.f && m <= 3.0e38f) frexpf(m, &e);                  // m in [2^(e-1), 2^e)
    const int k = m > 0.f && m <= 3.0e38f ? min(max(14 - e, -120), 120) : 0;   // (non-finite weights: the host keeps bf16x3)
    fac[co] = ldexpf(1.f, -(k + kF2XExp));
}

__global__ void pack_weights_f16x2_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                          const float* __restrict__ fac, uint16_t* __restrict__ wpk, int cout, int cin,
                                          int taps, int K16, int NT, int layout, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = i & 7;
    const int lane = (i >> 3) & 63;
    long t = i >> 9;
    const int nt = t % NT; t /= NT;
    const int k16 = t % K16; t /= K16;
    const int tap = (int)t;
    const int co = nt * 32 + (lane & 31);
    const int ci = k16 * 16 + (lane >> 5) * 8 + j;
    float v = 0.f;
    if (co < cout && ci < cin) {
        v = conv3d_weight_src(w, layout, co, ci, tap, cout, cin, taps, nullptr);
        if (scale != nullptr) v *= scale[co];
        v *= 0.5f / fac[co];                                      // 2^k[co]: exact
    }
    const _Float16 hi = (_Float16)v;
    wpk[i] = __builtin_bit_cast(uint16_t, hi);
    wpk[i + total] = __builtin_bit_cast(uint16_t, (_Float16)((float)hi * (1.f / 2048.f)));
    wpk[i + 2 * total] = __builtin_bit_cast(uint16_t, (_Float16)(v - (float)hi));
}

struct VariantB {
    int MT, NT, WM, WN, KS;
    // [0] fp32 in / fp32 out, [1] bf16 in / bf16 out, [2] fp32 with the 3-way bf16 split, [3] fp32 with the 2-term fp16 split (or null)
    void (*kern[4])(const ConvBP);
};

#define OCCD_VARIANT_B(MT, NT, WM, WN) \
    VariantB { MT, NT, WM, WN, 1, { conv3d_bf16_kernel<MT, NT, WM, WN, false, false>, conv3d_bf16_kernel<MT, NT, WM, WN, true, true>, nullptr, nullptr } }
#define OCCD_VARIANT_B3(MT, NT, WM, WN) \
    VariantB { MT, NT, WM, WN, 1, { conv3d_bf16_kernel<MT, NT, WM, WN, false, false>, conv3d_bf16_kernel<MT, NT, WM, WN, true, true>, \
                                    conv3d_bf16_kernel<MT, NT, WM, WN, false, false, 3>, conv3d_bf16_kernel<MT, NT, WM, WN, false, false, 2> } }

const VariantB kVariantsB[] = {
    OCCD_VARIANT_B(4, 1, 4, 1),    // 0: M512 x N32
    OCCD_VARIANT_B3(2, 1, 4, 1),   // 1: M256 x N32
    OCCD_VARIANT_B3(1, 1, 4, 1),   // 2: M128 x N32
    OCCD_VARIANT_B(4, 2, 4, 1),    // 3: M512 x N64
    OCCD_VARIANT_B3(2, 2, 4, 1),   // 4: M256 x N64
    OCCD_VARIANT_B(4, 2, 2, 2),    // 5: M256 x N128
    OCCD_VARIANT_B3(2, 2, 2, 2),   // 6: M128 x N128
    OCCD_VARIANT_B3(1, 2, 2, 2),   // 7: M64  x N128
    // 8: M32 x N128 with either split and 4-way in-workgroup split-K (16 waves): small volumes with a long K
    VariantB { 1, 1, 1, 4, 4, { nullptr, nullptr, conv3d_bf16_kernel<1, 1, 1, 4, false, false, 3, 4>,
                                conv3d_bf16_kernel<1, 1, 1, 4, false, false, 2, 4> } },
};
constexpr int kNumVariantsB = sizeof(kVariantsB) / sizeof(kVariantsB[0]);

// Tile of mwg output positions as TY x TZ: the candidate that stages the fewest input rows per launch (halo + ragged
// edges) among those that fit LDS.  2-D images (Zo = W >> mwg) get a TY > 1 tile instead of a one-row strip.
bool plan_b(const occd_conv3d_args* a, const VariantB& v, int NTtot, Tiling* best, int rsb) {
    const int mwg = v.MT * v.WM * 32;
    bool found = false;
    int cands[16];
    int nc = 0;
    if (a->Zo <= mwg) cands[nc++] = a->Zo;                       // whole columns (the 3-D stack: Z = 4 ... 32)
    for (int tz = 8; tz <= mwg; tz *= 2)
        if (tz < a->Zo) cands[nc++] = tz;
    for (int i = 0; i < nc; ++i) {
        Tiling t;
        t.TZ = cands[i];
        t.TY = mwg / t.TZ;
        if (t.TY < 1) continue;
        if (t.TY > a->Yo) t.TY = a->Yo;
        t.YIN = (t.TY - 1) * a->sy + (a->ky - 1) * a->dy + 1;
        t.ZIN = (t.TZ - 1) * a->sz + (a->kz - 1) * a->dz + 1;
        t.ytiles = (a->Yo + t.TY - 1) / t.TY;
        t.ztiles = (a->Zo + t.TZ - 1) / t.TZ;
        t.lds = (size_t)t.YIN * t.ZIN * rsb * v.KS;
        const size_t red = (size_t)(v.KS - 1) * v.WM * v.WN * v.MT * v.NT * 4096;   // split-K reduction scratch
        if (red > t.lds) t.lds = red;
        const int nwg_n = v.NT * v.WN;
        t.ngroups = (NTtot + nwg_n - 1) / nwg_n;
        t.nwg = (long)a->Xo * t.ytiles * t.ztiles;
        if (t.lds > occd::kMaxConvLds || (long)t.YIN * t.ZIN >= 65536 || t.nwg >= (1L << 24)) continue;
        // staged rows per launch + idle M slots of a tile smaller than mwg (they still cost MFMA time)
        t.cost = (double)t.nwg * ((double)t.YIN * t.ZIN + 2.0 * (mwg - (double)t.TY * t.TZ));
        if (t.lds > 80 * 1024) t.cost *= 1.15;                   // one workgroup per CU instead of two
        if (!found || t.cost < best->cost) { *best = t; found = true; }
    }
    return found;
}

}  // namespace

extern "C" int64_t occd_packed_weight_bf16_elems(int32_t cout, int32_t cin, int32_t taps) {
    if (cout <= 0 || cin <= 0 || taps <= 0) return OCCD_EINVAL;
    const int64_t K16 = (cin + 15) / 16, NT = (cout + 31) / 32;
    return (int64_t)taps * K16 * NT * 512;
}

// tap_ofs == nullptr: layout 0 / 1 / 2 of a dense tensor; else layout 3, the gathered view (s_co, s_ci, tap_ofs[taps]).
// nsplit = 3: the hi | mid | lo images of the 3-way split, 3 * occd_packed_weight_bf16_elems() elements.
static int pack_bf16(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin, int32_t taps, int32_t layout,
                     int64_t s_co, int64_t s_ci, const int32_t* tap_ofs, int nsplit, void* stream) {
    const int64_t total = occd_packed_weight_bf16_elems(cout, cin, taps);
    if (total <= 0) return OCCD_EINVAL;
    occd::TapMap tm{};
    tm.s_co = s_co; tm.s_ci = s_ci;
    for (int i = 0; tap_ofs != nullptr && i < taps; ++i) tm.ofs[i] = tap_ofs[i];
    const int K16 = (cin + 15) / 16, NT = (cout + 31) / 32;
    const int th = 256;
    const long blocks = (total + th - 1) / th;
    occd::ProfScope prof("pack_weights_bf16", (hipStream_t)stream, 0.0, (double)total * 6);
    hipLaunchKernelGGL(pack_weights_bf16_kernel, dim3((unsigned)blocks), dim3(th), 0, (hipStream_t)stream, w, scale,
                       (uint16_t*)wpk, cout, cin, taps, K16, NT, layout, (long)total, nsplit, tm);
    return occd::check_launch();
}

static int pack_bf16_dense(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin, int32_t kx, int32_t ky,
                           int32_t kz, int32_t layout, int nsplit, void* stream) {
    if (!w || !wpk || layout < 0 || layout > 2 || (layout == 2 && kx * ky * kz != 1)) return OCCD_EINVAL;
    return pack_bf16(w, scale, wpk, cout, cin, kx * ky * kz, layout, 0, 0, nullptr, nsplit, stream);
}

static int pack_bf16_gather(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin, int32_t ntaps,
                            int64_t s_co, int64_t s_ci, const int32_t* tap_ofs, int nsplit, void* stream) {
    if (!w || !wpk || !tap_ofs || ntaps <= 0 || ntaps > occd::kMaxTaps) return OCCD_EINVAL;
    return pack_bf16(w, scale, wpk, cout, cin, ntaps, 3, s_co, s_ci, tap_ofs, nsplit, stream);
}

extern "C" int occd_pack_weights_bf16(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                      int32_t kx, int32_t ky, int32_t kz, int32_t layout, void* stream) {
    return pack_bf16_dense(w, scale, wpk, cout, cin, kx, ky, kz, layout, 1, stream);
}

// three images (hi | mid | lo): the weight operand of the 3-way split
extern "C" int occd_pack_weights_bf16x3(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                        int32_t kx, int32_t ky, int32_t kz, int32_t layout, void* stream) {
    return pack_bf16_dense(w, scale, wpk, cout, cin, kx, ky, kz, layout, 3, stream);
}

extern "C" int occd_pack_weights_bf16_gather(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                             int32_t ntaps, int64_t s_co, int64_t s_ci, const int32_t* tap_ofs,
                                             void* stream) {
    return pack_bf16_gather(w, scale, wpk, cout, cin, ntaps, s_co, s_ci, tap_ofs, 1, stream);
}

// the hi | mid | lo images of the gathered operator: the 3-way split of the data-gradient operators (float32-accurate dgrad
// of the head convolutions on K2s3 in the fp32 training mode)
extern "C" int occd_pack_weights_bf16x3_gather(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                               int32_t ntaps, int64_t s_co, int64_t s_ci, const int32_t* tap_ofs,
                                               void* stream) {
    return pack_bf16_gather(w, scale, wpk, cout, cin, ntaps, s_co, s_ci, tap_ofs, 3, stream);
}

extern "C" int64_t occd_packed_weight_f16x2_bytes(int32_t cout, int32_t cin, int32_t taps) {
    const int64_t n = occd_packed_weight_bf16_elems(cout, cin, taps);
    if (n <= 0) return OCCD_EINVAL;
    return 3 * n * 2 + (int64_t)((cout + 31) / 32) * 32 * 4;
}

extern "C" int occd_pack_weights_f16x2(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                       int32_t kx, int32_t ky, int32_t kz, int32_t layout, void* stream) {
    if (!w || !wpk || layout < 0 || layout > 2 || (reinterpret_cast<uintptr_t>(wpk) & 15)) return OCCD_EINVAL;
    const int taps = kx * ky * kz;
    const int64_t total = occd_packed_weight_bf16_elems(cout, cin, taps);
    if (total <= 0 || (layout == 2 && taps != 1)) return OCCD_EINVAL;
    const int K16 = (cin + 15) / 16, NT = (cout + 31) / 32;
    float* const fac = reinterpret_cast<float*>(static_cast<uint16_t*>(wpk) + 3 * total);
    const int th = 256;
    const long blocks = (total + th - 1) / th;
    occd::ProfScope prof("pack_weights_f16x2", (hipStream_t)stream, 0.0, (double)total * 10);
    hipLaunchKernelGGL(f16x2_scale_kernel, dim3((unsigned)NT), dim3(32), 0, (hipStream_t)stream, w, scale, fac, cout, cin, taps,
                       NT, layout);
    hipLaunchKernelGGL(pack_weights_f16x2_kernel, dim3((unsigned)blocks), dim3(th), 0, (hipStream_t)stream, w, scale, fac,
                       (uint16_t*)wpk, cout, cin, taps, K16, NT, layout, (long)total);
    return occd::check_launch();
}

// `a->in`, `a->out`, `a->res1`, `a->res2` point at fp32 or bf16 channels-last rows -- all four the same type --, `a->wpk`
// at the image of occd_pack_weights_bf16, `a->bias` at fp32.  *_cs / *_coff count ELEMENTS.  The `dtype` argument of the
// two entry points is a mode, OCCD_CONV_* of the header, one row of kModesB each:
// F32 / BF16 = bf16 operands from float32 / bfloat16 tensors.
// BF16X3 = float32 tensors with the 3-way bf16 split of both operands (wpk from occd_pack_weights_bf16x3): float32-level
// accuracy on the bf16 matrix pipe, an opt-in experiment beside the exact-fp32 kernels.
// F16X2_HEAD = float32 tensors with the two-term fp16 split (wpk from occd_pack_weights_f16x2): the head convolutions on
// K2s3h (conv3d_c32p.hip) only; any other geometry is rejected (OCCD_EINVAL), there is no generic form.
// F16X2 = float32 tensors with the two-term fp16 split on this kernel (K2bh; wpk from occd_pack_weights_f16x2): any
// geometry K2b takes, act_in NONE or RELU.
namespace {

constexpr unsigned kActRelu = 1u << OCCD_ACT_NONE | 1u << OCCD_ACT_RELU;
// (input sigmoid: the CRP products sigmoid(P_logits) @ mega, CRP3D.py:80 -- float32 operands with the 3-way split only)
constexpr occd::ConvStorage kF32 = {4, 4, kActRelu}, kF32Sigmoid = {4, 4, kActRelu | 1u << OCCD_ACT_SIGMOID};
constexpr occd::ConvStorage kBf16 = {2, 8, kActRelu};     // 16-byte staging loads: 8 bf16 / 4 (+4) floats

struct ModeB {
    occd::ConvStorage st;     // the activation tensors
    int ksel;                 // column of kVariantsB[].kern (-1: no kernel here)
    int rsb;                  // LDS row stride of that kernel's staging
    const char* name;         // profile row of a plain launch ...
    const char* name_phases;  // ... and of a merged phase launch
};
constexpr ModeB kModesB[] = {
    {kF32, 0, kRSB, "conv3d_bf16", "conv3d_bf16x3_phases"},                       // OCCD_CONV_F32
    {kBf16, 1, kRSB, "conv3d_bf16s", "conv3d_bf16x3_phases"},                     // OCCD_CONV_BF16
    {kF32Sigmoid, 2, kRSB3, "conv3d_bf16x3", "conv3d_bf16x3_phases"},             // OCCD_CONV_BF16X3
    {kF32, -1, 0, nullptr, nullptr},                                              // OCCD_CONV_F16X2_HEAD
    {kF32, 3, kRSB2, "conv3d_bf16x3_f16x2", "conv3d_bf16x3_phases_f16x2"},        // OCCD_CONV_F16X2
};
constexpr int kNumModesB = sizeof(kModesB) / sizeof(kModesB[0]);
static_assert(OCCD_CONV_F32 == 0 && OCCD_CONV_BF16 == 1 && OCCD_CONV_BF16X3 == 2 && OCCD_CONV_F16X2_HEAD == 3 &&
              OCCD_CONV_F16X2 == 4 && kNumModesB == 5, "kModesB is indexed by OCCD_CONV_*");

// n phases (n = 1: a plain launch) that differ only in wpk, kx / ky / kz and o_off_*: ONE launch
int launch_b(const occd_conv3d_args* a, int n, int32_t mode, hipStream_t stream) {
    const ModeB& m = kModesB[mode];
    const int ksel = m.ksel;
    if (ksel < 0) return OCCD_EINVAL;
    const int cin16 = (a->cin + 15) & ~15;
    const int NTtot = (a->cout + 31) / 32;
    const occd_conv3d_args big = occd::conv3d_widest_phase(a, n);
    const long copies = (long)a->batch * n;
    int order[kNumVariantsB];
    int no = 0;
    if (a->tile_hint > 0 && a->tile_hint <= kNumVariantsB) {
        order[no++] = a->tile_hint - 1;
    } else if (NTtot == 1) {
        order[no++] = 0; order[no++] = 1; order[no++] = 2;
    } else if (NTtot == 2) {
        order[no++] = 3; order[no++] = 4; order[no++] = 6; order[no++] = 7;
    } else {
        order[no++] = 5; order[no++] = 6; order[no++] = 7;
    }
    int pick = -1;
    Tiling til{};
    for (int i = 0; i < no; ++i) {
        Tiling t{};
        if (kVariantsB[order[i]].kern[ksel] == nullptr) continue;
        if (!plan_b(&big, kVariantsB[order[i]], NTtot, &t, m.rsb)) continue;
        pick = order[i];
        til = t;
        if (t.nwg * t.ngroups * copies >= 512) break;   // else keep refining to the finest fit
    }
    if (pick < 0) return OCCD_ENOMEM;
    if (ksel >= 2 && a->tile_hint == 0 && til.nwg * til.ngroups * copies <= 320 && cin16 >= 128 && NTtot % 4 == 0) {
        // too few output tiles to fill the chip: multiply the waves by splitting K inside the workgroup (K2's rule)
        Tiling t{};
        if (plan_b(&big, kVariantsB[8], NTtot, &t, m.rsb) && t.nwg * t.ngroups * copies <= 1024) {
            pick = 8;
            til = t;
        }
    }
    const VariantB& v = kVariantsB[pick];

    ConvBP p{};
    p.cin16 = cin16;
    p.K16tot = cin16 / 16;
    const occd::ConvLaunch L = {n > 1 ? m.name_phases : m.name, v.WM * v.WN * v.KS * 64, (size_t)m.rsb * v.KS, m.st, 2.0, false};
    return occd::conv3d_launch(a, n, til, v.kern[ksel], p, L, [&](PhaseBP& ph, const occd_conv3d_args& ai) {
        ph.wpk = (const u32x4*)ai.wpk;
        // the trailer of the fp16 image: after its three images of taps * K16 * NT * 512 halves each
        ph.fac = ksel == 3 ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(ai.wpk) +
                                                            3 * (size_t)ai.kx * ai.ky * ai.kz * (cin16 / 16) * NTtot * 512)
                           : nullptr;
    }, stream);
}

}  // namespace

extern "C" int occd_conv3d_bf16_fwd(const occd_conv3d_args* a, int32_t dtype, void* stream) {
    if (dtype < 0 || dtype >= kNumModesB) return OCCD_EINVAL;
    const int bad = occd::conv3d_validate(a, kModesB[dtype].st);
    if (bad != OCCD_OK) return bad;
    if (dtype == OCCD_CONV_F16X2_HEAD) {   // K2s3h: the head launches only
        const int r = occd::try_conv3d_c32_slide_x3(a, (hipStream_t)stream, true);
        return r < 0 ? r : r == 0 ? OCCD_EINVAL : OCCD_OK;
    }
    if (dtype == OCCD_CONV_BF16X3) {   // the full-resolution head launches: sliding-window form of the split (K2s3, conv3d_c32p.hip)
        const int r = occd::try_conv3d_c32_slide_x3(a, (hipStream_t)stream);
        if (r != 0) return r < 0 ? r : OCCD_OK;
    }
    return launch_b(a, 1, dtype, (hipStream_t)stream);
}

// The n in {1, 2, 4, 8} sub-pixel phases of ONE transposed convolution on K2b as one launch (the bf16-pipe twin of
// occd_conv3d_fwd_phases, same contract: a[0..n) differ ONLY in wpk, kx / ky / kz and o_off_*).
extern "C" int occd_conv3d_bf16_fwd_phases(const occd_conv3d_args* a, int32_t n, int32_t dtype, void* stream) {
    if (dtype < 0 || dtype >= kNumModesB || dtype == OCCD_CONV_F16X2_HEAD) return OCCD_EINVAL;
    const int bad = occd::conv3d_validate_phases(a, n, kModesB[dtype].st);
    if (bad != OCCD_OK) return bad;
    return launch_b(a, n, dtype, (hipStream_t)stream);
}
