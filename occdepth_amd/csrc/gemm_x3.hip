// K16 -- row-major float32 GEMM on the bf16 matrix pipe with the 3-way operand split (the library GEMMs
// of the 2-D network -- tap GEMMs of the decoder levels, Winograd-domain products at 1/8 and 1/16, expand 1x1 convolutions of
// the 1/16 and 1/32 encoder stages -- out of the eval path):
//
//   C[b][m][n] = act( sum_k A[b][m][k] * B[b][k][n] + bias[m] )        A: M x K, k contiguous;  B: K x N, n contiguous
//
// Both operands are float32 in memory and are split x = hi + mid + lo (three bf16 terms, 24 significant bits) WHILE they
// are staged into LDS; six v_mfma_f32_32x32x16_bf16 per 16-k step -- (mid,mid), (hi,lo), (lo,hi), (hi,mid), (mid,hi),
// (hi,hi), smallest first -- reproduce the float32 product to ~2^-24 relative (the same arithmetic as K2s3 / K2b SPLIT=3):
// float32-level accuracy at 6/16 of the fp32-MFMA time, so nothing needs pre-packing and weights stay the plain tensors.
// Layout in LDS: A rows [hi 32 k | mid | lo | 16 B pad] = 208 B (13 sixteen-byte slots, odd: conflict-free ds_read_b128
// of 8 consecutive k per lane); B as it lies in memory, [term][k][n] with rows of TN bf16 + 64 B pad (row stride = 64 mod
// 128 B), read with the transposing ds_read_b64_tr_b16 of gfx950 (lane <- 4 consecutive k of ONE column; layout pinned on
// hardware by tools/probe_bf16.hip and used by K8b): no transposition pass, no 2-byte scatter.
// One K step = 32 k: global -> registers (prefetched under the MFMAs of the previous step) -> split -> LDS, two barriers.
// Workgroup = WM x WN waves, a wave owns MT x NT tiles of 32 x 32; D layout: lane -> column n, registers -> rows m, so every
// store instruction writes two 128-byte row segments.  Block order is XCD-aware: an XCD walks a contiguous range of tiles
// with the index over the SMALLER operand's reuse dimension fastest, so the larger operand's tile is fetched once per L2.
//
// Reference semantics replaced: torch.matmul / torch.bmm / F.conv2d(1x1) call sites of occdepth/models/unet2d.py:24-46,137-165
// (through the tap-GEMM / Winograd-domain forms of this repo's unet2d.py) and the geffnet MBConv expand convolutions.
#include <cstdlib>
#include <type_traits>
#include <vector>
#include "device.h"

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // rows of odd length: dword-aligned 16-byte loads

namespace {

struct GemmP {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    const float* res;                   // optional: + res[b][m][n] (laid out like C) after bias / activation
    const float* kscale;                // optional: B[b][k][n] * kscale[b][k] (the squeeze-excite gate of a project convolution)
    const float* bias_n = nullptr;      // optional: + bias_n[b][n] ahead of the activation (K16's barrier-phased kernels only)
    long s_bias_n = 0;                  // floats between the batch items of bias_n (0 = shared)
    int M, N, K;
    long lda, ldb, ldc, sA, sB, sC;     // elements
    int act;                            // 0 none, 1 swish, 2 leaky relu (slope)
    int act_a;                          // 1: sigmoid applied to the A elements while they are staged (CRP: sigmoid(P_logits) @ mega)
    float slope;
    int mtiles, ntiles, n_fast;         // n_fast: the N-tile index runs fastest in the block order (A tile reused), else M
    int mr_tiles;                       // K16p: 32-row tiles per row range (mtiles = the number of ranges)
    unsigned nwg;
    const float* fac = nullptr;         // f16x2 image (pre = 4): 2^-(k[m] + kF2XExp) per row of the FIRST batch item's image
    long s_fac = 0;                     // floats between the batch items' factors (0 = shared image)
};

constexpr int kARow = 208;              // bytes per A row in LDS: 3 x 64 B (32 k of one term) + 16 B pad

// (the splits split3_bf16x8 / split3_bf16x4 and the transposed fragment read tr_frag_bf16x8: device.h)

// PRE: 0 = both operands float32 in memory (split while staged); 1 = A is the pre-split fragment image of
// occd_gemm_x3_pack (weights: [row tile 32][k16][term][lane][8 bf16], read straight from L2 like K2b's weights -- no LDS,
// no split arithmetic, no ds_write for that operand); 2 = B is (role 1 image: [column tile 32][k16][term][lane][8]).
// TERMS: 3 = the split (float32-level accuracy); 1 = plain bf16 operands, ONE MFMA per 16-k step (the bf16 training mode,
// BASELINE configs[3]: "bf16 MFMA, fp32 storage and accumulate" like K2b): same staging and layout, only the hi plane is
// written and read; 2 = the two-term fp16 split (PRE = 1 only: A is the image of occd_gemm_f16x2_pack, [row tile 32][k16][hi, lo]
// [lane][8 fp16] of w' = 2^k[m] w; B is staged as 2^kF2XExp x = hi + 2^-11 lo' in TWO fp16 planes; three
// v_mfma_f32_32x32x16_f16 per 16-k step -- (lo_a, hi_b), (hs_a, lo'_b), (hi_a, hi_b) with hs = 2^-11 hi formed in registers -- and
// the epilogue multiplies by fac[m] = 2^-(k[m] + kF2XExp) ahead of the bias: the numerics of K2s3h / K2bh, conv3d_c32p.hip).
// KS > 1: in-workgroup split-K (the long-K / few-pixel project convolutions: 96 ... 230 output tiles for 256 CUs and K = 960 ...
// 3840).  The KS wave groups of a workgroup own the same output tile, take interleaved 32-k steps (each group with its own LDS
// stage), and their accumulators meet in LDS once, after the loop; group 0 runs the epilogue.  16 waves per CU instead of 4:
// while one group waits at its split / LDS round trip, the others issue MFMAs.
template <int MT, int NT, int WM, int WN, int PRE, int TERMS = 3, int KS = 1>
__global__ void __launch_bounds__(WM* WN * 64 * KS) gemm_x3_kernel(const GemmP p) {
    static_assert(KS == 1 || PRE == 0, "split-K stages both operands");
    static_assert(TERMS != 2 || PRE == 1, "the fp16 split reads A from its pre-scaled image");
    constexpr int NPL = TERMS == 2 ? 2 : 3;         // term planes of the B tile in LDS / terms per record of the A image
    constexpr int NTH = WM * WN * 64, TM = WM * MT * 32, TN = WN * NT * 32;
    constexpr int SB = TN * 2 + 64;                 // bytes per B row (one k, one term): = 64 mod 128
    constexpr int BTERM = 32 * SB;                  // bytes per term of the B tile
    constexpr int NA = TM * 4 / NTH;                // A staging items per thread: (row, 8-k chunk), 2 float4 each
    constexpr int NB = 8 * TN / NTH;                // B staging items per thread: (k row, 4-column chunk), 1 float4 each
    static_assert(TM * 4 % NTH == 0 && 8 * TN % NTH == 0, "staging split");
    // Register prefetch depth: K steps whose global loads are in flight while one is multiplied.  Measured with 4 steps on the
    // 64 x 64 tile and 2 on 128 x 64 (round 4, session 31): SLOWER on every short-K launch (48 -> 288 on 28365 pixels 34 -> 38.5
    // us, 384 -> 2304 on 468 pixels 23 -> 26 us; 160 VGPRs instead of 112), and the long-K project convolution on 96 workgroups
    // stayed at 80 us: memory latency is not what a step of a small tile waits for (split arithmetic + LDS round trip + two
    // barriers are).  So 1 everywhere; the loop keeps the general form.
    constexpr int PF = 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    constexpr int STAGE = (PRE == 1 ? 0 : TM * kARow) + (PRE == 2 ? 0 : NPL * BTERM);   // LDS bytes of one K group
    const int kg = KS == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / NTH);   // K group of this wave
    unsigned char* const lA = glds + kg * STAGE;
    unsigned char* const lB = lA + (PRE == 1 ? 0 : TM * kARow);

    const int tid = threadIdx.x - kg * NTH;          // thread index inside the K group
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, h = lane >> 5, i16 = lane & 15, g1 = (lane >> 4) & 1;

    const uint32_t bid = xcd_remap(blockIdx.x, p.nwg);   // an XCD walks a contiguous run of tiles
    int mt_i, nt_i;
    if (p.n_fast) { nt_i = bid % p.ntiles; mt_i = bid / p.ntiles; }
    else { mt_i = bid % p.mtiles; nt_i = bid / p.mtiles; }
    const int bz = blockIdx.y;
    const int m0 = mt_i * TM, n0 = nt_i * TN;
    const float* const Ab = p.A + (size_t)bz * p.sA;
    const float* const Bb = p.B + (size_t)bz * p.sB;

    // staging descriptors
    size_t a_off[NA];
    int a_dst[NA], a_k[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int f = tid + i * NTH;
        const int row = f >> 2, c8 = f & 3;
        a_off[i] = (size_t)min(m0 + row, p.M - 1) * p.lda + c8 * 8;
        a_dst[i] = row * kARow + c8 * 16;
        a_k[i] = c8 * 8;
    }
    size_t b_col[NB];
    int b_dst[NB], b_k[NB], b_sh[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int f = tid + i * NTH;
        const int k = f / (TN / 4), c4 = f - k * (TN / 4);
        // a chunk that crosses the end of the row loads the row's LAST four columns instead and is shifted into place
        // while it is committed (no read beyond the tensor, no branch around the load)
        b_col[i] = (size_t)min(n0 + c4 * 4, p.N - 4);
        b_sh[i] = n0 + c4 * 4 - (int)b_col[i];                     // 0, or 1 .. 3 (partial chunk), or >= 4 (columns >= N: never stored)
        b_dst[i] = k * SB + c4 * 8;
        b_k[i] = k;
    }

    f32x4 ra[PF][NA][2], rb[PF][NB];
    float rg[PF][NB];                                // kscale of the staged B rows (1 without)
    const float* const Gb = p.kscale != nullptr ? p.kscale + (size_t)bz * p.K : nullptr;
    // FAST (interior tiles of a K % 32 == 0 problem -- all but the last column of tiles): no address clamps, no K / N tail
    // selects; the general form pays ~2 extra VALU instructions per MFMA for them (PMC: 5.8 VALU per MFMA)
    auto issue = [&](int u, int k0, auto fast_c) {   // global -> register set u for the K step starting at k0
        constexpr bool FAST = decltype(fast_c)::value;
        if (PRE != 1) {
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int k = FAST ? k0 + a_k[i] : min(k0 + a_k[i], p.K - 8);
                const float* src = Ab + a_off[i] - a_k[i] + k;
                ra[u][i][0] = *(const f32x4*)src;
                ra[u][i][1] = *(const f32x4*)(src + 4);
            }
        }
        if (PRE != 2) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int k = FAST ? k0 + b_k[i] : min(k0 + b_k[i], p.K - 1);
                rb[u][i] = *(const f32x4u*)(Bb + (size_t)k * p.ldb + b_col[i]);
                rg[u][i] = Gb != nullptr ? Gb[k] : 1.f;     // (uniform branch; the load rides with the tile's own)
            }
        }
    };
    auto commit = [&](int u, int k0, auto fast_c) {  // register set u -> split -> LDS
        constexpr bool FAST = decltype(fast_c)::value;
#pragma unroll
        for (int i = 0; i < (PRE == 1 ? 0 : NA); ++i) {
            const bool ok = FAST || k0 + a_k[i] < p.K;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            u32x4 hi, mid, lo;
            f32x4 a0 = ra[u][i][0], a1 = ra[u][i][1];
            if (p.act_a) {                                   // (launch-uniform branch: the CRP products only)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a0[j] = 1.f / (1.f + __expf(-a0[j]));
                    a1[j] = 1.f / (1.f + __expf(-a1[j]));
                }
            }
            split3_bf16x8(ok ? a0 : z, ok ? a1 : z, hi, mid, lo);
            *(u32x4*)(lA + a_dst[i]) = hi;
            if (TERMS == 3) {
                *(u32x4*)(lA + a_dst[i] + 64) = mid;
                *(u32x4*)(lA + a_dst[i] + 128) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < (PRE == 2 ? 0 : NB); ++i) {
            f32x4 v;
            if (FAST) {
                v = rb[u][i] * rg[u][i];
            } else {
                const bool ok = k0 + b_k[i] < p.K;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                const f32x4 w = ok ? rb[u][i] * rg[u][i] : z;
                const int sh = b_sh[i];                  // (selects, not branches: the shift is lane-dependent)
                v.x = sh == 0 ? w.x : sh == 1 ? w.y : sh == 2 ? w.z : w.w;
                v.y = sh == 0 ? w.y : sh == 1 ? w.z : sh == 2 ? w.w : 0.f;
                v.z = sh == 0 ? w.z : sh == 1 ? w.w : 0.f;
                v.w = sh == 0 ? w.w : 0.f;
            }
            u32x2 hi, mid, lo;
            if (TERMS == 2) {
                split2_f16x4(v, hi, lo);
                *(u32x2*)(lB + b_dst[i]) = hi;
                *(u32x2*)(lB + BTERM + b_dst[i]) = lo;
                continue;
            }
            split3_bf16x4(v, hi, mid, lo);
            *(u32x2*)(lB + b_dst[i]) = hi;
            if (TERMS == 3) {
                *(u32x2*)(lB + BTERM + b_dst[i]) = mid;
                *(u32x2*)(lB + 2 * BTERM + b_dst[i]) = lo;
            }
        }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

    // lane-constant LDS offsets: A row of this lane (8 consecutive k of half h); B transposed read (row 8 h + (i16 >> 2),
    // 4 columns 16 g1 + 4 (i16 & 3) of the 32-column tile; second read 4 rows further)
    int a_lane[MT], b_lane[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a_lane[mt] = ((wm * MT + mt) * 32 + li) * kARow + h * 16;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
        b_lane[nt] = (8 * h + (i16 >> 2)) * SB + ((wn * NT + nt) * 32 + 16 * g1 + 4 * (i16 & 3)) * 2;

#define OCCD_GX3(WT, XT)                                                                                              \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[mt][nt] =  \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[mt][WT]), bf[nt][XT], acc[mt][nt], 0, 0, 0)
#define OCCD_GX3H(W, XT)                                                                                              \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[mt][nt] =  \
        __builtin_amdgcn_mfma_f32_32x32x16_f16(W, __builtin_bit_cast(f16x8, bf[nt][XT]), acc[mt][nt], 0, 0, 0)

    // pre-split operand: fragment records of this wave's tiles, one K16 sub-step ahead of the MFMAs
    const int K16tot = (p.K + 15) >> 4;
    const u32x4* pk[PRE == 1 ? MT : PRE == 2 ? NT : 1];
    if (PRE == 1) {
        const u32x4* base = reinterpret_cast<const u32x4*>(p.A) + (size_t)bz * p.sA + lane;       // sA: u32x4 per batch item
        const int last = (p.M + 31) / 32 - 1;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) pk[mt] = base + (size_t)min(m0 / 32 + wm * MT + mt, last) * K16tot * (64 * NPL);
    } else if (PRE == 2) {
        const u32x4* base = reinterpret_cast<const u32x4*>(p.B) + (size_t)bz * p.sB + lane;
        const int last = (p.N + 31) / 32 - 1;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) pk[nt] = base + (size_t)min(n0 / 32 + wn * NT + nt, last) * K16tot * 192;
    }
    constexpr int NPK = PRE == 1 ? MT : PRE == 2 ? NT : 1;
    // two fragment sets: the 16-k sub-step `ks` of a step uses set ks and then requests the same sub-step of the NEXT 32-k step
    // into it -- a full step (two barriers, 48 MFMAs per wave on the 256 x 128 tile) ahead.  (Round 4 requested ONE sub-step ahead
    // into a single set; its ISA waits for the fragments a few instructions after requesting them: vmcnt(0) in front of every
    // sub-step's MFMAs -- an L2 round trip per 16 k, which is why the pre-split form never beat splitting on the fly.)
    u32x4 pn[2][NPK][NPL];
    auto fetch_pk = [&](int slot, int k16) {
        const int kc = min(k16, K16tot - 1);      // (a step past K multiplies the other operand's zeros)
#pragma unroll
        for (int i = 0; i < NPK; ++i)
#pragma unroll
            for (int t = 0; t < NPL; ++t) pn[slot][i][t] = pk[i][(kc * NPL + t) * 64];
    };

    const int ksteps = (p.K + 31) >> 5;
    auto kloop = [&](auto fast_c) {
    // step s of the workgroup's walk belongs to K group s % KS; every group joins every barrier
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (u * KS + kg < ksteps) issue(u, (u * KS + kg) * 32, fast_c);
    if (PRE != 0) {
        fetch_pk(0, 0);
        fetch_pk(1, 1);
    }
    for (int s0 = 0; s0 < ksteps; s0 += PF * KS) {
#pragma unroll
    for (int u = 0; u < PF; ++u) {                  // (unrolled: the register set of a step is a compile-time index)
        const int s = s0 + u * KS + kg;
        if (s0 + u * KS >= ksteps) continue;        // (workgroup-uniform)
        const bool active = KS == 1 || s < ksteps;  // (uniform per K group)
        __syncthreads();                // previous tile consumed
        if (active) commit(u, s * 32, fast_c);
        __syncthreads();
        // (pre-split forms: the request is unconditional, from a clamped step -- behind a branch the compiler cannot count the
        //  fragment loads in flight across it and waits for all of them)
        if (PRE != 0 && KS == 1) issue(u, min(s + PF * KS, ksteps - 1) * 32, fast_c);
        else if (s + PF * KS < ksteps) issue(u, (s + PF * KS) * 32, fast_c);
        if (!active) continue;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 af[MT][3];
            bf16x8 bf[NT][3];
            if (PRE == 1) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int t = 0; t < NPL; ++t) af[mt][t] = pn[ks][mt][t];
            } else {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int t = 0; t < TERMS; ++t) af[mt][t] = *(const u32x4*)(lA + a_lane[mt] + t * 64 + ks * 32);
            }
            if (PRE == 2) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int t = 0; t < 3; ++t) bf[nt][t] = __builtin_bit_cast(bf16x8, pn[ks][nt][t]);
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int t = 0; t < TERMS; ++t) bf[nt][t] = tr_frag_bf16x8(lB + t * BTERM + b_lane[nt] + ks * 16 * SB, 4 * SB);
            }
            if (PRE != 0) fetch_pk(ks, s * 2 + ks + 2);
            if (TERMS == 2) {                     // smallest terms first: (lo_a, hi_b), (hs_a, lo'_b), (hi_a, hi_b)
                f16x8 ahs[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) ahs[mt] = __builtin_bit_cast(f16x8, af[mt][0]) * (_Float16)(1.f / 2048.f);
                OCCD_GX3H(__builtin_bit_cast(f16x8, af[mt][TERMS == 2 ? 1 : 0]), 0);
                OCCD_GX3H(ahs[mt], TERMS == 2 ? 1 : 0);
                OCCD_GX3H(__builtin_bit_cast(f16x8, af[mt][0]), 0);
                continue;
            }
            if (TERMS == 3) {
                OCCD_GX3(1, 1);
                OCCD_GX3(0, TERMS == 3 ? 2 : 0);
                OCCD_GX3(TERMS == 3 ? 2 : 0, 0);
                OCCD_GX3(0, 1);
                OCCD_GX3(1, 0);
            }
            OCCD_GX3(0, 0);
        }
    }
    }
    };
    if ((p.K & 31) == 0 && n0 + TN <= p.N) kloop(std::true_type{});
    else kloop(std::false_type{});
#undef OCCD_GX3
#undef OCCD_GX3H

    if (KS > 1) {
        // sum the K groups' accumulators through LDS (the stages are dead after the barrier), group 0 stores
        float* red = reinterpret_cast<float*>(glds);
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

    // f16x2: acc *= fac[m] = 2^-(k[m] + kF2XExp) (exact), ahead of everything the epilogue adds.  A pass of its own, fenced: the 16
    // factors of a row tile (registers r <-> rows (r & 3) + 8 (r >> 2) + 4 h: four 16-byte loads, the factors are padded to whole row
    // tiles) are dead before the epilogue's bias loads and row addresses go live.
    if (TERMS == 2) {
        const float* const Fb = p.fac + (size_t)bz * p.s_fac;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int mb = m0 + (wm * MT + mt) * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 f4 = *(const f32x4*)(Fb + min(mb + 8 * g, ((p.M + 31) & ~31) - 4));      // (rows >= M: never stored)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[mt][nt][4 * g + i] *= f4[i];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // bias along N (ABI 13: one value per COLUMN -- a lane is a column, so one load per tile column; rows-times-weights
    // products whose rows are voxels / pixels: the CRP's relation-logit convolutions), added ahead of the activation
    if (p.bias_n != nullptr) {                                  // (uniform branch)
        const float* bnp = p.bias_n + (size_t)bz * p.s_bias_n;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float bnv = bnp[min(n0 + (wn * NT + nt) * 32 + li, p.N - 1)];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] += bnv;
        }
    }
    // epilogue: lane -> column n, registers -> rows (r & 3) + 8 (r >> 2) + 4 h.  Bias / activation are uniform over the
    // launch: one straight-line store sequence per combination
    float* const Cb = p.C + (size_t)bz * p.sC;
    const float* const Rb = p.res != nullptr ? p.res + (size_t)bz * p.sC : nullptr;
    auto store_all = [&](auto has_bias, auto act_sel) {
        constexpr bool BIAS = decltype(has_bias)::value;
        constexpr int ACT = decltype(act_sel)::value;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = n0 + (wn * NT + nt) * 32 + li;
            const bool n_ok = n < p.N;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int mb = m0 + (wm * MT + mt) * 32 + 4 * h;
                float bv[16];
                if (BIAS) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) bv[r] = p.bias[min(mb + (r & 3) + 8 * (r >> 2), p.M - 1)];
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mb + (r & 3) + 8 * (r >> 2);
                    float v = acc[mt][nt][r];
                    if (BIAS) v += bv[r];
                    if (ACT == 1) v = occd::swish_fast(v);
                    else if (ACT == 2) v = v > 0.f ? v : v * p.slope;
                    if (n_ok && m < p.M) {
                        if (Rb != nullptr) v += Rb[(size_t)m * p.ldc + n];       // (uniform branch)
                        Cb[(size_t)m * p.ldc + n] = v;
                    }
                }
            }
        }
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    if (p.bias == nullptr && p.act == 0) store_all(F_{}, std::integral_constant<int, 0>{});
    else if (p.bias != nullptr && p.act == 1) store_all(T_{}, std::integral_constant<int, 1>{});
    else if (p.bias != nullptr && p.act == 2) store_all(T_{}, std::integral_constant<int, 2>{});
    else if (p.bias != nullptr) store_all(T_{}, std::integral_constant<int, 0>{});
    else if (p.act == 1) store_all(F_{}, std::integral_constant<int, 1>{});
    else store_all(F_{}, std::integral_constant<int, 2>{});
}

// ------------------------------------------------------------------------------------------------
// K16w -- the same GEMM, wave-specialised (PRE = 0 only): 256 x 128 tile, 8 waves = 4 MFMA waves (one per SIMD, each owns
// 64 rows x all 128 columns: 2 x 4 tiles, 128 accumulator registers) + 4 LOADER waves (one per SIMD) that do nothing but
// global -> split -> LDS for the NEXT 16-k step into the other half of a double-buffered LDS tile.  In the barrier-phased
// kernel above every wave splits, then every wave multiplies: the matrix pipe idles through ~55 % of a K step
// (profiles/r04_gemm_x3_v1.txt: 150 TF/s = 36 % of the bf16 peak issued).  Here the split arithmetic and the ds_writes of
// a loader wave issue in the shadow of the MFMAs of the wave it shares a SIMD with; one barrier per 16-k step.
constexpr int kWsTM = 256, kWsTN = 128;
constexpr int kWsARow = 112;                         // A row of ONE 16-k step: 3 x 32 B + 16 B pad (7 slots, odd)
constexpr int kWsSB = kWsTN * 2 + 64;                // B row (one k, one term)
constexpr int kWsBTerm = 16 * kWsSB;
constexpr int kWsStage = kWsTM * kWsARow + 3 * kWsBTerm;   // 28,672 + 15,360 = 44,032 B per buffer

// DBG (development A/B, wrong results, only with -DOCCD_GEMM_DEV_VARIANTS): 1 = truncate instead of split (what does the split
// arithmetic cost?), 2 = loaders skip the global loads (what does memory cost?), 3 = MFMA waves read LDS in step 0 only (what do
// the fragment reads cost?), 4 = loaders only keep the barriers (what does the whole loader cost?), 5 = no barriers at all in the K loop (what do the barriers cost?)
template <int DBG>
__global__ void __launch_bounds__(512, 2) gemm_x3_ws_kernel(const GemmP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool loader = wave >= 4;                   // waves 0-3 multiply, 4-7 load (one of each per SIMD)
    const int li = lane & 31, h = lane >> 5, i16 = lane & 15, g1 = (lane >> 4) & 1;

    const uint32_t bid = xcd_remap(blockIdx.x, p.nwg);
    int mt_i, nt_i;
    if (p.n_fast) { nt_i = bid % p.ntiles; mt_i = bid / p.ntiles; }
    else { mt_i = bid % p.mtiles; nt_i = bid / p.mtiles; }
    const int bz = blockIdx.y;
    const int m0 = mt_i * kWsTM, n0 = nt_i * kWsTN;
    const int K16tot = (p.K + 15) >> 4;

    if (loader) {
        // ---------------------------------------------------------------- loader waves: 256 threads
        const int lt = tid - 256;
        const float* const Ab = p.A + (size_t)bz * p.sA;
        const float* const Bb = p.B + (size_t)bz * p.sB;
        // A: 256 rows x 2 chunks of 8 k = 512 items -> 2 per thread; B: 16 k rows x 32 column chunks = 512 items -> 2 per thread
        size_t a_off[2], b_col[2];
        int a_dst[2], a_k[2], b_dst[2], b_k[2], b_sh[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int f = lt + i * 256;
            const int row = f >> 1, c8 = f & 1;
            a_off[i] = (size_t)min(m0 + row, p.M - 1) * p.lda;
            a_dst[i] = row * kWsARow + c8 * 16;
            a_k[i] = c8 * 8;
            const int k = f >> 5, c4 = f & 31;
            b_col[i] = (size_t)min(n0 + c4 * 4, p.N - 4);
            b_sh[i] = n0 + c4 * 4 - (int)b_col[i];
            b_dst[i] = k * kWsSB + c4 * 8;
            b_k[i] = k;
        }
        // TWO register sets: the loads of step s + 3 are issued while step s + 1 is committed, so every load has two full
        // steps (~2 x 1.8k cycles) to come back -- one step was not enough once the B panel of an XCD's tile run stops fitting
        // its 4 MB L2 (PMC, profiles/r04_pmc_gemm_head_v1.txt: 417 MB fetched for 48 MB of operands, MFMA pipe busy 40 %)
        f32x4 ra[2][2][2], rb[2][2];
        auto loader = [&](auto fast_c) {             // FAST: interior tile of a K % 16 == 0 problem (no clamps, no tail selects)
        constexpr bool FAST = decltype(fast_c)::value;
        auto issue = [&](int k0, int set) {
            if (DBG == 2 && k0 > 16) return;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float* src = Ab + a_off[i] + (FAST ? k0 + a_k[i] : min(k0 + a_k[i], p.K - 8));
                ra[set][i][0] = *(const f32x4*)src;
                ra[set][i][1] = *(const f32x4*)(src + 4);
                rb[set][i] = *(const f32x4u*)(Bb + (size_t)(FAST ? k0 + b_k[i] : min(k0 + b_k[i], p.K - 1)) * p.ldb + b_col[i]);
            }
        };
        auto commit = [&](int k0, int set, unsigned char* buf) {
            unsigned char* const lB = buf + kWsTM * kWsARow;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const bool oka = FAST || k0 + a_k[i] < p.K;
                u32x4 hi, mid, lo;
                if (DBG == 1) {
                    const f32x4 x0 = ra[set][i][0], x1 = ra[set][i][1];
                    hi = u32x4{__builtin_amdgcn_perm(__float_as_uint(x0.y), __float_as_uint(x0.x), 0x07060302u),
                               __builtin_amdgcn_perm(__float_as_uint(x0.w), __float_as_uint(x0.z), 0x07060302u),
                               __builtin_amdgcn_perm(__float_as_uint(x1.y), __float_as_uint(x1.x), 0x07060302u),
                               __builtin_amdgcn_perm(__float_as_uint(x1.w), __float_as_uint(x1.z), 0x07060302u)};
                    mid = hi; lo = hi;
                } else {
                    split3_bf16x8(oka ? ra[set][i][0] : z, oka ? ra[set][i][1] : z, hi, mid, lo);
                }
                *(u32x4*)(buf + a_dst[i]) = hi;
                *(u32x4*)(buf + a_dst[i] + 32) = mid;
                *(u32x4*)(buf + a_dst[i] + 64) = lo;
                f32x4 v;
                const f32x4 w = (FAST || k0 + b_k[i] < p.K) ? rb[set][i] : z;
                if (FAST) {
                    v = w;
                } else {
                    const int sh = b_sh[i];
                    v.x = sh == 0 ? w.x : sh == 1 ? w.y : sh == 2 ? w.z : w.w;
                    v.y = sh == 0 ? w.y : sh == 1 ? w.z : sh == 2 ? w.w : 0.f;
                    v.z = sh == 0 ? w.z : sh == 1 ? w.w : 0.f;
                    v.w = sh == 0 ? w.w : 0.f;
                }
                u32x2 h2, m2, l2;
                if (DBG == 1) {
                    h2 = u32x2{__builtin_amdgcn_perm(__float_as_uint(w.y), __float_as_uint(w.x), 0x07060302u),
                               __builtin_amdgcn_perm(__float_as_uint(w.w), __float_as_uint(w.z), 0x07060302u)};
                    m2 = h2; l2 = h2;
                } else {
                    split3_bf16x4(v, h2, m2, l2);
                }
                *(u32x2*)(lB + b_dst[i]) = h2;
                *(u32x2*)(lB + kWsBTerm + b_dst[i]) = m2;
                *(u32x2*)(lB + 2 * kWsBTerm + b_dst[i]) = l2;
            }
        };
        // step t lives in register set t & 1 and LDS buffer t & 1
        issue(0, 0);
        if (K16tot > 1) issue(16, 1);
        commit(0, 0, glds);                          // step 0 -> buffer 0
        if (K16tot > 2) issue(32, 0);
        __syncthreads();
        for (int s = 0; s < K16tot; s += 2) {        // unrolled by two: the register-set index is a compile-time constant
            if (DBG == 4) {
                __syncthreads();
                if (s + 1 >= K16tot) break;
                __syncthreads();
                continue;
            }
            if (DBG == 5) continue;
            if (s + 1 < K16tot) {
                commit((s + 1) * 16, 1, glds + kWsStage);
                if (s + 3 < K16tot) issue((s + 3) * 16, 1);
            }
            __syncthreads();                         // buffer 1 published, buffer 0 consumed
            if (s + 1 >= K16tot) break;
            if (s + 2 < K16tot) {
                commit((s + 2) * 16, 0, glds);
                if (s + 4 < K16tot) issue((s + 4) * 16, 0);
            }
            __syncthreads();                         // buffer 0 published, buffer 1 consumed
        }
        };
        if ((p.K & 15) == 0 && n0 + kWsTN <= p.N) loader(std::true_type{});
        else loader(std::false_type{});
        return;
    }

    // -------------------------------------------------------------------- MFMA waves: wave w owns rows 64 w .. 64 w + 63
    f32x16 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    int a_lane[2], b_lane[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) a_lane[mt] = ((wave * 2 + mt) * 32 + li) * kWsARow + h * 16;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) b_lane[nt] = kWsTM * kWsARow + (8 * h + (i16 >> 2)) * kWsSB + (nt * 32 + 16 * g1 + 4 * (i16 & 3)) * 2;

#define OCCD_WS(WT, XT)                                                                                          \
    _Pragma("unroll") for (int mt = 0; mt < 2; ++mt) _Pragma("unroll") for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[mt][WT]), bf[nt][XT], acc[mt][nt], 0, 0, 0)

    __syncthreads();                                 // buffer 0 published
    u32x4 af[2][3];
    bf16x8 bf[4][3];
    for (int s = 0; s < K16tot; ++s) {
        const unsigned char* buf = glds + (s & 1) * kWsStage;
        if (DBG != 3 || s == 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int t = 0; t < 3; ++t) af[mt][t] = *(const u32x4*)(buf + a_lane[mt] + t * 32);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int t = 0; t < 3; ++t) bf[nt][t] = tr_frag_bf16x8(buf + t * kWsBTerm + b_lane[nt], 4 * kWsSB);
        }
        OCCD_WS(1, 1);
        OCCD_WS(0, 2);
        OCCD_WS(2, 0);
        OCCD_WS(0, 1);
        OCCD_WS(1, 0);
        OCCD_WS(0, 0);
        if (DBG != 5) __syncthreads();
    }
#undef OCCD_WS

    float* const Cb = p.C + (size_t)bz * p.sC;
    auto store_all = [&](auto has_bias, auto act_sel) {
        constexpr bool BIAS = decltype(has_bias)::value;
        constexpr int ACT = decltype(act_sel)::value;
        // One 32-row block at a time, fenced: with all 128 accumulators live the compiler otherwise hoists the 128 bias loads
        // and 64-bit row addresses of every block above the first store (round 4: 44 spilled VGPRs / 180 B of scratch in this
        // epilogue -- VERDICT r4 weak #6).  Row pointers advance by additions from one base per block.
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            __builtin_amdgcn_sched_barrier(0);
            const int mb = m0 + (wave * 2 + mt) * 32 + 4 * h;
            float bv[16];
            if (BIAS) {
#pragma unroll
                for (int r = 0; r < 16; ++r) bv[r] = p.bias[min(mb + (r & 3) + 8 * (r >> 2), p.M - 1)];
            }
            float* const row0 = Cb + (size_t)mb * p.ldc + n0 + li;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dm = (r & 3) + 8 * (r >> 2);
                if (mb + dm >= p.M) continue;                 // (wave-half uniform)
                float* const row = row0 + (size_t)dm * p.ldc;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    float v = acc[mt][nt][r];
                    if (BIAS) v += bv[r];
                    if (ACT == 1) v = occd::swish_fast(v);
                    else if (ACT == 2) v = v > 0.f ? v : v * p.slope;
                    if (n0 + nt * 32 + li < p.N) row[nt * 32] = v;
                }
            }
        }
    };
    using T_ = std::true_type;
    using F_ = std::false_type;
    if (p.bias == nullptr && p.act == 0) store_all(F_{}, std::integral_constant<int, 0>{});
    else if (p.bias != nullptr && p.act == 1) store_all(T_{}, std::integral_constant<int, 1>{});
    else if (p.bias != nullptr && p.act == 2) store_all(T_{}, std::integral_constant<int, 2>{});
    else if (p.bias != nullptr) store_all(T_{}, std::integral_constant<int, 0>{});
    else if (p.act == 1) store_all(F_{}, std::integral_constant<int, 1>{});
    else store_all(F_{}, std::integral_constant<int, 2>{});
}

// ------------------------------------------------------------------------------------------------
// K16p -- panel-stationary form for SHORT K with pre-split weights (PRE = 1 operands; K <= 848): the expand convolutions of
// the MBConv stages and the tap GEMM of the 1/1 decoder level (K = 32 ... 224).  The barrier-phased kernel above re-stages
// and re-splits the same B columns once per 64 ... 256 rows of A and spends two barriers per 32 k; with K this short a
// workgroup is mostly prologue.  Here a workgroup owns a 64- (or 32-) column panel of B over the WHOLE K: staged + split into
// LDS once ([k][hi | mid | lo][64 columns] + 64 B: 448 B per k, two workgroups per CU up to K = 176, K <= 352 fits), ONE barrier, and then its 8 waves walk the row tiles of A (MT x 32 rows each,
// fragments of the pre-split image straight from L2, one 16-k step ahead) against the resident panel -- no barrier and no
// split arithmetic in the K loop, B fragments by ds_read_b64_tr_b16 as in K16.  The grid is (column panels) x (row ranges);
// the host cuts M into ranges only as far as it needs workgroups for 256 CUs.
// LDS bytes per k of a panel of NT x 32 columns: [hi | mid | lo] x (64 NT) B, + 64 B for NT = 2: 192 / 448, both = 64 mod 128
// (conflict-free transposing reads).  NT = 1 (32 columns): twice the panels for the few-pixel stages (468 / 1848 pixels), K up
// to 848, at twice the weight-fragment traffic per MFMA -- which a launch that small does not notice.
// SPLIT = 2 (the f16x2 image, pre = 4; numerics above gemm_x3_kernel): [hi | lo'] x (64 NT) B + 64 B for EITHER width -- 192 / 320,
// again 64 mod 128.  The 32-column row keeps its 192 bytes (same K limit, 848); the 64-column row shrinks from 448 to 320.
constexpr int panel_row_bytes(int nt, int split = 3) {
    return split == 2 ? 2 * 64 * nt + 64 : 3 * 64 * nt + (nt == 1 ? 0 : 64);
}
// Development probe (tools/panel_timeline.cpp builds this file with -DOCCD_PANEL_TIMELINE; never in libocc_hip.so): the shader
// clock of every wave of ONE workgroup at the phase boundaries of the kernel below.
#ifdef OCCD_PANEL_TIMELINE
__device__ unsigned long long g_panel_tl[8 * 64];
__device__ int g_panel_probe_wg = 0;
#define OCCD_TL(idx)                                                                                                   \
    do {                                                                                                               \
        if ((int)blockIdx.x == g_panel_probe_wg && blockIdx.y == 0 && lane == 0 && (idx) < 64)                         \
            g_panel_tl[wave * 64 + (idx)] = __builtin_amdgcn_s_memtime();                                              \
    } while (0)
#else
#define OCCD_TL(idx) do { } while (0)
#endif
constexpr int kPanelPass = 6;                         // float4 loads in flight per thread while the panel is staged
template <int MT, int NT, int PD, int SPLIT = 3>
__global__ void __launch_bounds__(512) gemm_x3_panel_kernel(const GemmP p) {
    constexpr int TN = 32 * NT, SB = panel_row_bytes(NT, SPLIT), TB = 64 * NT, C4 = TN / 4;   // TB: bytes of one term's columns in a row
    constexpr int NPL = SPLIT;                            // terms per weight record / term planes of a panel row
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, h = lane >> 5, i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int K16tot = (p.K + 15) >> 4, KP = K16tot * 16;

    const uint32_t bid = xcd_remap(blockIdx.x, p.nwg);
    const int nt_i = bid % p.ntiles, mr_i = bid / p.ntiles;       // column panel fastest: an XCD shares the row range's weights
    const int bz = blockIdx.y;
    const int n0 = nt_i * TN;
    const int tiles_all = (p.M + 31) >> 5;
    const int t0 = mr_i * p.mr_tiles, t1 = min(t0 + p.mr_tiles, tiles_all);   // 32-row tiles of this workgroup

    // weight fragments of this wave's row tile, PD 16-k steps ahead of the MFMAs (a step is 6 MT NT MFMAs = 0.1 ... 0.2 us of
    // matrix time against ~1 us of L2 latency; one workgroup per CU on the few-pixel launches, so nothing else hides it); the
    // first PD steps are requested before the panel is staged
    const u32x4* const Abase = reinterpret_cast<const u32x4*>(p.A) + (size_t)bz * p.sA + lane;
    const u32x4* pk[MT];
    u32x4 an[PD][MT][NPL];
    auto fetch_a = [&](int d, int k16) {
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int t = 0; t < NPL; ++t) an[d][j][t] = pk[j][(k16 * NPL + t) * 64];
    };
    auto first_a = [&](int tb) {
#pragma unroll
        for (int j = 0; j < MT; ++j) pk[j] = Abase + (size_t)min(tb + j, tiles_all - 1) * K16tot * (64 * NPL);
#pragma unroll
        for (int d = 0; d < PD; ++d)
            fetch_a(d, min(d, K16tot - 1));
    };
    OCCD_TL(0);                                            // kernel entry
    if (t0 + wave * MT < t1) first_a(t0 + wave * MT);
    OCCD_TL(1);                                            // first weight fragments requested

    // ---- the B panel: (k, 4-column chunk) items, C4 per k row; kPanelPass loads in flight per thread, then split -> LDS
    {
        const float* const Bb = p.B + (size_t)bz * p.sB;
        const int total = KP * C4;
        const bool edge = n0 + TN > p.N;
        // (all loads of a pass in flight before the first split: K <= 192 is ONE pass, one HBM round trip)
        for (int base = 0; base < total; base += 512 * kPanelPass) {
            f32x4 v[kPanelPass];
#pragma unroll
            for (int i = 0; i < kPanelPass; ++i) {
                const int f = base + i * 512 + tid;
                const int k = min(f / C4, p.K - 1), c = min(n0 + (f % C4) * 4, p.N - 4);
                v[i] = *(const f32x4u*)(Bb + (size_t)k * p.ldb + c);
            }
            OCCD_TL(2);                                    // panel loads of this pass requested
#pragma unroll
            for (int i = 0; i < kPanelPass; ++i) {
                const int f = base + i * 512 + tid;
                const int k = f / C4, c4 = f % C4;
                if (f >= total) continue;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                f32x4 w = k < p.K ? v[i] : z;
                if (edge) {                              // (workgroup-uniform: the last panel of a row only)
                    const int sh = n0 + c4 * 4 - min(n0 + c4 * 4, p.N - 4);
                    const f32x4 u = w;
                    w.x = sh == 0 ? u.x : sh == 1 ? u.y : sh == 2 ? u.z : u.w;
                    w.y = sh == 0 ? u.y : sh == 1 ? u.z : sh == 2 ? u.w : 0.f;
                    w.z = sh == 0 ? u.z : sh == 1 ? u.w : 0.f;
                    w.w = sh == 0 ? u.w : 0.f;
                }
                u32x2 hi, mid, lo;
                unsigned char* dst = glds + k * SB + c4 * 8;
                if (SPLIT == 2) {
                    split2_f16x4(w, hi, lo);
                    *(u32x2*)dst = hi;
                    *(u32x2*)(dst + TB) = lo;
                } else {
                    split3_bf16x4(w, hi, mid, lo);
                    *(u32x2*)dst = hi;
                    *(u32x2*)(dst + TB) = mid;
                    *(u32x2*)(dst + 2 * TB) = lo;
                }
            }
        }
    }
    OCCD_TL(3);                                           // panel split and written (this wave's share)
    __syncthreads();
    OCCD_TL(4);                                            // panel complete
    int b_lane[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_lane[nt] = (8 * h + (i16 >> 2)) * SB + (nt * 32 + 16 * g1 + 4 * (i16 & 3)) * 2;
    float* const Cb = p.C + (size_t)bz * p.sC;
    const float* const Fb = SPLIT == 2 ? p.fac + (size_t)bz * p.s_fac : nullptr;

    for (int tb = t0 + wave * MT; tb < t1; tb += 8 * MT) {
        f32x16 acc[MT][NT];
#pragma unroll
        for (int j = 0; j < MT; ++j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][nt][r] = 0.f;
        bf16x8 bn[NT][NPL];
        auto fetch_b = [&](int k16) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int t = 0; t < NPL; ++t) bn[nt][t] = tr_frag_bf16x8(glds + t * TB + b_lane[nt] + k16 * 16 * SB, 4 * SB);
        };
        fetch_b(0);
#define OCCD_GP(WT, XT)                                                                                              \
    _Pragma("unroll") for (int j = 0; j < MT; ++j) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[j][nt] =    \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[j][WT]), bf[nt][XT], acc[j][nt], 0, 0, 0)
#define OCCD_GPH(W, XT)                                                                                              \
    _Pragma("unroll") for (int j = 0; j < MT; ++j) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[j][nt] =    \
        __builtin_amdgcn_mfma_f32_32x32x16_f16(W, __builtin_bit_cast(f16x8, bf[nt][XT]), acc[j][nt], 0, 0, 0)
        // One 16-k step on fragment set d (a compile-time index).  Requests are UNCONDITIONAL and come from clamped addresses (the
        // last steps re-read the last fragments): behind a branch the compiler cannot count the loads in flight and waits for
        // vmcnt(0) at the join -- every step then pays a full L2 round trip however deep the prefetch (tools/panel_timeline.cpp:
        // ~700 cycles per step of 192 MFMA cycles; the ISA of the branchy form had `s_waitcnt vmcnt(0)` in front of every step).
        auto step = [&](int k16, int d, bool more_a) {        // (always inlined into unrolled loops: d, more_a are constants there)
            u32x4 af[MT][3];
            bf16x8 bf[NT][3];
#pragma unroll
            for (int t = 0; t < NPL; ++t) {
#pragma unroll
                for (int j = 0; j < MT; ++j) af[j][t] = an[d][j][t];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bf[nt][t] = bn[nt][t];
            }
            if (tb == t0 + wave * MT) OCCD_TL(8 + k16);      // step k16 of the first row tile: operands in registers
            if (more_a) fetch_a(d, min(k16 + PD, K16tot - 1));
            fetch_b(min(k16 + 1, K16tot - 1));
            if constexpr (SPLIT == 2) {                      // smallest terms first: (lo_a, hi_b), (hs_a, lo'_b), (hi_a, hi_b)
                f16x8 ahs[MT];
#pragma unroll
                for (int j = 0; j < MT; ++j) ahs[j] = __builtin_bit_cast(f16x8, af[j][0]) * (_Float16)(1.f / 2048.f);
                OCCD_GPH(__builtin_bit_cast(f16x8, af[j][1]), 0);
                OCCD_GPH(ahs[j], 1);
                OCCD_GPH(__builtin_bit_cast(f16x8, af[j][0]), 0);
            } else {
                OCCD_GP(1, 1);
                OCCD_GP(0, 2);
                OCCD_GP(2, 0);
                OCCD_GP(0, 1);
                OCCD_GP(1, 0);
                OCCD_GP(0, 0);
            }
        };
        // main loop: whole groups of PD steps, NO branch inside the body (exact vmcnt counts); then the < PD remaining steps,
        // whose fragments are already on their way
        int k0 = 0;
        for (; k0 + PD <= K16tot; k0 += PD) {
#pragma unroll
            for (int d = 0; d < PD; ++d) step(k0 + d, d, true);
        }
#pragma unroll
        for (int d = 0; d < PD - 1; ++d)
            if (k0 + d < K16tot) step(k0 + d, d, false);
#undef OCCD_GP
#undef OCCD_GPH
        // the next row tile's first fragments go out BEFORE this tile's stores (loads return in order among loads; queued behind
        // the stores they would wait for them to drain)
        if (tb + 8 * MT < t1) first_a(tb + 8 * MT);
        if (tb == t0 + wave * MT) OCCD_TL(5);              // K loop of the first row tile issued
        // f16x2: acc *= fac[m] = 2^-(k[m] + kF2XExp) (exact) in a fenced pass of its own, as in K16 (row tiles < t1 only: their
        // factors exist, four 16-byte loads per tile)
        if (SPLIT == 2) {
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                const int mb = min(tb + j, tiles_all - 1) * 32 + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 f4 = *(const f32x4*)(Fb + mb + 8 * g);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[j][nt][4 * g + i] *= f4[i];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // epilogue of this tile set: lane -> column, registers -> rows (as K16)
        auto store_all = [&](auto has_bias, auto act_sel) {
            constexpr bool BIAS = decltype(has_bias)::value;
            constexpr int ACT = decltype(act_sel)::value;
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                if (tb + j >= t1) continue;                              // (wave-uniform: a row tile of the next range / past M)
                const int mb = (tb + j) * 32 + 4 * h;
                float bv[16];
                if (BIAS) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) bv[r] = p.bias[min(mb + (r & 3) + 8 * (r >> 2), p.M - 1)];
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int n = n0 + nt * 32 + li;
                    const bool n_ok = n < p.N;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int m = mb + (r & 3) + 8 * (r >> 2);
                        float v = acc[j][nt][r];
                        if (BIAS) v += bv[r];
                        if (ACT == 1) v = occd::swish_fast(v);
                        else if (ACT == 2) v = v > 0.f ? v : v * p.slope;
                        if (n_ok && m < p.M) Cb[(size_t)m * p.ldc + n] = v;
                    }
                }
            }
        };
        using T_ = std::true_type;
        using F_ = std::false_type;
        if (p.bias == nullptr && p.act == 0) store_all(F_{}, std::integral_constant<int, 0>{});
        else if (p.bias != nullptr && p.act == 1) store_all(T_{}, std::integral_constant<int, 1>{});
        else if (p.bias != nullptr && p.act == 2) store_all(T_{}, std::integral_constant<int, 2>{});
        else if (p.bias != nullptr) store_all(T_{}, std::integral_constant<int, 0>{});
        else if (p.act == 1) store_all(F_{}, std::integral_constant<int, 1>{});
        else store_all(F_{}, std::integral_constant<int, 2>{});
        if (tb == t0 + wave * MT) OCCD_TL(6);              // stores of the first row tile issued
    }
    OCCD_TL(7);                                            // last instruction of the wave
}

// ------------------------------------------------------------------------------------------------
// K21 -- K16p cut along K over SEVERAL workgroups (round 6): the project convolutions of the 1/16 and 1/32 encoder stages,
// `bn(conv1x1(y * gate)) + skip` with K = 960 ... 3840 input channels, 160 ... 640 output channels and 2 x 468 / 2 x 1848
// pixels (geffnet MBConv behind occdepth/models/unet2d.py:188-196).  A 64 x 64 tiling gives 90 ... 230 output tiles for 256 CUs, each
// walking the whole K behind two barriers per 32 k (K16: 56 us; the in-workgroup split-K form: 39 ... 56 us; K11s, exact fp32:
// 35 us) for 1.7 ... 4.6 GFLOP -- 47 ... 57 TF/s.  Here the grid is (32-column panels of B) x (row ranges) x (batch) x (K chunks
// of <= 416 k): every workgroup stages + splits ITS K chunk of its panel once (the gate multiplies the rows while they are
// staged, rounded to float32 first like the reference's x * gate), ONE barrier, then its 8 waves walk the row tiles against the
// resident chunk with pre-split weight fragments straight from L2 -- K16p's loop, no barrier, no split arithmetic -- and store
// the float32 PARTIAL tile into a workspace [b][z][M][ld]; `splitk_reduce_kernel` sums the z partials in index order
// (deterministic), adds the BatchNorm shift, the activation and the skip.  Two launches, both with hundreds of workgroups.
struct GemmSKP {
    GemmP g;
    int k16_per_z;                      // 16-k steps per K chunk (the last chunk may be shorter, never empty)
    float* ws;                          // partial sums
    long ld_ws, z_stride, b_stride;     // floats: row pitch (multiple of 32), between K chunks, between batch items
};

// SPLIT = 2: the f16x2 image (pre = 4).  The partial tiles stay in the scaled domain; `splitk_reduce_kernel` multiplies the SUM
// by fac[m] -- once per output, where a factor at the partial store would cost nz multiplications (both are exact).
template <int NT, int PD, int SPLIT = 3>
__global__ void __launch_bounds__(512) gemm_x3_panel_splitk_kernel(const GemmSKP q) {
    const GemmP& p = q.g;
    constexpr int TN = 32 * NT, SB = panel_row_bytes(NT, SPLIT), TB = 64 * NT, C4 = TN / 4;
    constexpr int NPL = SPLIT;
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, h = lane >> 5, i16 = lane & 15, g1 = (lane >> 4) & 1;
    const int K16tot = (p.K + 15) >> 4;
    const int kz = blockIdx.z;
    const int ks0 = kz * q.k16_per_z;                           // first 16-k step of this chunk
    const int nst = min(q.k16_per_z, K16tot - ks0);             // its steps (>= 1 by construction of the grid)
    const int kbase = ks0 * 16;

    const uint32_t bid = xcd_remap(blockIdx.x, p.nwg);
    const int nt_i = bid % p.ntiles, mr_i = bid / p.ntiles;
    const int bz = blockIdx.y;
    const int n0 = nt_i * TN;
    const int tiles_all = (p.M + 31) >> 5;
    const int t0 = mr_i * p.mr_tiles, t1 = min(t0 + p.mr_tiles, tiles_all);

    const u32x4* const Abase = reinterpret_cast<const u32x4*>(p.A) + (size_t)bz * p.sA + (size_t)ks0 * (64 * NPL) + lane;
    const u32x4* pk;
    u32x4 an[PD][NPL];
    auto fetch_a = [&](int d, int k16) {
#pragma unroll
        for (int t = 0; t < NPL; ++t) an[d][t] = pk[(k16 * NPL + t) * 64];
    };
    auto first_a = [&](int tb) {
        pk = Abase + (size_t)min(tb, tiles_all - 1) * K16tot * (64 * NPL);
#pragma unroll
        for (int d = 0; d < PD; ++d) fetch_a(d, min(d, nst - 1));
    };
    if (t0 + wave < t1) first_a(t0 + wave);

    // ---- this chunk of the B panel: (k, 4-column chunk) items; all loads of a pass in flight before the first split
    {
        const float* const Bb = p.B + (size_t)bz * p.sB;
        const float* const ksc = p.kscale != nullptr ? p.kscale + (size_t)bz * p.K : nullptr;
        const int total = nst * 16 * C4;
        const bool edge = n0 + TN > p.N;
        for (int base = 0; base < total; base += 512 * kPanelPass) {
            f32x4 v[kPanelPass];
            float sc[kPanelPass];
#pragma unroll
            for (int i = 0; i < kPanelPass; ++i) {
                const int f = base + i * 512 + tid;
                const int k = min(kbase + f / C4, p.K - 1), c = min(n0 + (f % C4) * 4, p.N - 4);
                v[i] = *(const f32x4u*)(Bb + (size_t)k * p.ldb + c);
                sc[i] = ksc != nullptr ? ksc[k] : 1.f;
            }
#pragma unroll
            for (int i = 0; i < kPanelPass; ++i) {
                const int f = base + i * 512 + tid;
                const int k = f / C4, c4 = f % C4;
                if (f >= total) continue;
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                f32x4 w = kbase + k < p.K ? v[i] : z;
                if (ksc != nullptr) w *= sc[i];                 // (one rounding to float32: the reference's x * gate)
                if (edge) {
                    const int sh = n0 + c4 * 4 - min(n0 + c4 * 4, p.N - 4);
                    const f32x4 u = w;
                    w.x = sh == 0 ? u.x : sh == 1 ? u.y : sh == 2 ? u.z : u.w;
                    w.y = sh == 0 ? u.y : sh == 1 ? u.z : sh == 2 ? u.w : 0.f;
                    w.z = sh == 0 ? u.z : sh == 1 ? u.w : 0.f;
                    w.w = sh == 0 ? u.w : 0.f;
                }
                u32x2 hi, mid, lo;
                unsigned char* dst = glds + k * SB + c4 * 8;
                if (SPLIT == 2) {
                    split2_f16x4(w, hi, lo);
                    *(u32x2*)dst = hi;
                    *(u32x2*)(dst + TB) = lo;
                } else {
                    split3_bf16x4(w, hi, mid, lo);
                    *(u32x2*)dst = hi;
                    *(u32x2*)(dst + TB) = mid;
                    *(u32x2*)(dst + 2 * TB) = lo;
                }
            }
        }
    }
    __syncthreads();
    int b_lane[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_lane[nt] = (8 * h + (i16 >> 2)) * SB + (nt * 32 + 16 * g1 + 4 * (i16 & 3)) * 2;
    float* const Cb = q.ws + (size_t)bz * q.b_stride + (size_t)kz * q.z_stride;

    for (int tb = t0 + wave; tb < t1; tb += 8) {
        f32x16 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
        bf16x8 bn[NT][NPL];
        auto fetch_b = [&](int k16) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int t = 0; t < NPL; ++t) bn[nt][t] = tr_frag_bf16x8(glds + t * TB + b_lane[nt] + k16 * 16 * SB, 4 * SB);
        };
        fetch_b(0);
#define OCCD_GP(WT, XT)                                                                                              \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[nt] =                                                      \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[WT]), bf[nt][XT], acc[nt], 0, 0, 0)
#define OCCD_GPH(W, XT)                                                                                              \
    _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[nt] =                                                      \
        __builtin_amdgcn_mfma_f32_32x32x16_f16(W, __builtin_bit_cast(f16x8, bf[nt][XT]), acc[nt], 0, 0, 0)
        // (requests unconditional from clamped steps, branch-free groups of PD steps: see K16p)
        auto step = [&](int k16, int d, bool more_a) {
            u32x4 af[3];
            bf16x8 bf[NT][3];
#pragma unroll
            for (int t = 0; t < NPL; ++t) {
                af[t] = an[d][t];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) bf[nt][t] = bn[nt][t];
            }
            if (more_a) fetch_a(d, min(k16 + PD, nst - 1));
            fetch_b(min(k16 + 1, nst - 1));
            if constexpr (SPLIT == 2) {                      // (lo_a, hi_b), (hs_a, lo'_b), (hi_a, hi_b)
                const f16x8 ahs = __builtin_bit_cast(f16x8, af[0]) * (_Float16)(1.f / 2048.f);
                OCCD_GPH(__builtin_bit_cast(f16x8, af[1]), 0);
                OCCD_GPH(ahs, 1);
                OCCD_GPH(__builtin_bit_cast(f16x8, af[0]), 0);
            } else {
                OCCD_GP(1, 1);
                OCCD_GP(0, 2);
                OCCD_GP(2, 0);
                OCCD_GP(0, 1);
                OCCD_GP(1, 0);
                OCCD_GP(0, 0);
            }
        };
        int k0 = 0;
        for (; k0 + PD <= nst; k0 += PD) {
#pragma unroll
            for (int d = 0; d < PD; ++d) step(k0 + d, d, true);
        }
#pragma unroll
        for (int d = 0; d < PD - 1; ++d)
            if (k0 + d < nst) step(k0 + d, d, false);
#undef OCCD_GP
#undef OCCD_GPH
        if (tb + 8 < t1) first_a(tb + 8);
        // partial tile: lane -> column, registers -> rows; the workspace rows are 128-byte aligned (ld_ws % 32 == 0)
        const int mb = tb * 32 + 4 * h;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n = n0 + nt * 32 + li;
            const bool n_ok = n < q.ld_ws;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mb + (r & 3) + 8 * (r >> 2);
                if (n_ok && m < p.M) Cb[(size_t)m * q.ld_ws + n] = acc[nt][r];
            }
        }
    }
}

// out[b][m][n] = act(fac[m] * sum_z ws[b][z][m][n] + bias[m]) + res[b][m][n]; z in index order; fac: the row factors of an f16x2
// weight image, or NULL (bf16x3: no factor).  One thread = 4 consecutive n.
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                            const float* __restrict__ bias, const float* __restrict__ res,
                                                            int M, int N, int nz, long ld_ws, long z_stride, long b_stride,
                                                            long ldc, long sC, int act, float slope, int vec_ok,
                                                            const float* __restrict__ fac) {
    const int n4 = (N + 3) >> 2;
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (long)M * n4) return;
    const int m = (int)(item / n4), n = (int)(item - (long)m * n4) * 4;
    const int b = blockIdx.y;
    const float* src = ws + (size_t)b * b_stride + (size_t)m * ld_ws + n;
    f32x4 s = *(const f32x4*)src;                               // (the pad columns of the workspace rows exist: ld_ws >= N rounded to 32)
    for (int z = 1; z < nz; ++z) s += *(const f32x4*)(src + (size_t)z * z_stride);
    if (fac != nullptr) s *= fac[m];                            // 2^-(k[m] + kF2XExp): exact
    if (bias != nullptr) s += bias[m];
    float v[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (act == 1) v[j] = occd::swish_fast(v[j]);
        else if (act == 2) v[j] = v[j] > 0.f ? v[j] : v[j] * slope;
    }
    const size_t o = (size_t)b * sC + (size_t)m * ldc + n;
    if (vec_ok && n + 3 < N) {
        f32x4 r = {v[0], v[1], v[2], v[3]};
        if (res != nullptr) r += *(const f32x4*)(res + o);
        *(f32x4*)(out + o) = r;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n + j < N) out[o + j] = v[j] + (res != nullptr ? res[o + j] : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
// K16t -- "NT" form for weight gradients: C[b][m][n] = sum_k A[b][m][k] * B[b][n][k], BOTH operands with k contiguous and
// of ANY dword alignment and any K (rows of H*W pixels: odd lengths are the rule).  dW of a pointwise convolution is
// gy (Cout x HW) . x^T (HW x Cin): both tensors lie k(= pixel)-contiguous in NCHW memory, so both are staged like K16's A
// operand (rows of [hi | mid | lo] 32 k, conflict-free ds_read_b128 fragments) -- no transposing reads, no transposed copy.
// The last K step masks element-wise (a per-lane branch that only the tail step takes).
template <int MT, int NT, int WM, int WN, int TERMS = 3>
__global__ void __launch_bounds__(WM* WN * 64) gemm_x3_nt_kernel(const GemmP p) {
    constexpr int NTH = WM * WN * 64, TM = WM * MT * 32, TN = WN * NT * 32;
    constexpr int NA = TM * 4 / NTH, NB = TN * 4 / NTH;
    static_assert(TM * 4 % NTH == 0 && TN * 4 % NTH == 0, "staging split");
    extern __shared__ __attribute__((aligned(16))) unsigned char glds[];
    unsigned char* const lA = glds;
    unsigned char* const lB = glds + TM * kARow;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave - wm * WN;
    const int li = lane & 31, h = lane >> 5;
    const int mt_i = blockIdx.x % p.mtiles, nt_i = blockIdx.x / p.mtiles;
    const int bz = blockIdx.y;
    const int m0 = mt_i * TM, n0 = nt_i * TN;
    const float* const Ab = p.A + (size_t)bz * p.sA;
    const float* const Bb = p.B + (size_t)bz * p.sB;
    // split-K over blockIdx.z: a weight gradient is a SMALL matrix (Cout x Cin) reduced over MANY pixels -- without the
    // split a 288 x 48 gradient at 93 x 305 pixels is 6 workgroups walking K = 28,365 alone.  Split z owns the 32-k steps
    // [z * p.act, (z + 1) * p.act) (p.act = steps per split) and writes its own partial C (summed by the caller).
    const int step0 = blockIdx.z * p.act;
    const int step1 = min(step0 + p.act, (p.K + 31) >> 5);

    const float* a_src[NA];
    const float* b_src[NB];
    int a_dst[NA], b_dst[NB];
    const int kc = (tid & 3) * 8;                          // this thread's 8-k chunk inside a 32-k step (same for all its items)
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int row = (tid + i * NTH) >> 2;
        a_src[i] = Ab + (size_t)min(m0 + row, p.M - 1) * p.lda + kc;
        a_dst[i] = row * kARow + (tid & 3) * 16;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int row = (tid + i * NTH) >> 2;
        b_src[i] = Bb + (size_t)min(n0 + row, p.N - 1) * p.ldb + kc;
        b_dst[i] = row * kARow + (tid & 3) * 16;
    }
    f32x4 ra[NA][2], rb[NB][2];
    auto load8 = [&](const float* src, int k0, f32x4 (&v)[2]) {
        const int rem = p.K - (k0 + kc);
        if (rem >= 8) {
            v[0] = *(const f32x4u*)(src + k0);
            v[1] = *(const f32x4u*)(src + k0 + 4);
        } else {                                           // tail step only
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = j < rem ? src[k0 + j] : 0.f;
            v[0] = f32x4{t[0], t[1], t[2], t[3]};
            v[1] = f32x4{t[4], t[5], t[6], t[7]};
        }
    };
    auto issue = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) load8(a_src[i], k0, ra[i]);
#pragma unroll
        for (int i = 0; i < NB; ++i) load8(b_src[i], k0, rb[i]);
    };
    auto commit = [&]() {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            u32x4 hi, mid, lo;
            split3_bf16x8(ra[i][0], ra[i][1], hi, mid, lo);
            *(u32x4*)(lA + a_dst[i]) = hi;
            if (TERMS == 3) {
                *(u32x4*)(lA + a_dst[i] + 64) = mid;
                *(u32x4*)(lA + a_dst[i] + 128) = lo;
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            u32x4 hi, mid, lo;
            split3_bf16x8(rb[i][0], rb[i][1], hi, mid, lo);
            *(u32x4*)(lB + b_dst[i]) = hi;
            if (TERMS == 3) {
                *(u32x4*)(lB + b_dst[i] + 64) = mid;
                *(u32x4*)(lB + b_dst[i] + 128) = lo;
            }
        }
    };
    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
    int a_lane[MT], b_lane[NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) a_lane[mt] = ((wm * MT + mt) * 32 + li) * kARow + h * 16;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) b_lane[nt] = ((wn * NT + nt) * 32 + li) * kARow + h * 16;

#define OCCD_GNT(WT, XT)                                                                                             \
    _Pragma("unroll") for (int mt = 0; mt < MT; ++mt) _Pragma("unroll") for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = \
        __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[mt][WT]), __builtin_bit_cast(bf16x8, bf[nt][XT]), acc[mt][nt], 0, 0, 0)
    issue(step0 * 32);
    for (int s = step0; s < step1; ++s) {
        __syncthreads();
        commit();
        __syncthreads();
        if (s + 1 < step1) issue((s + 1) * 32);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 af[MT][3], bf[NT][3];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int t = 0; t < TERMS; ++t) af[mt][t] = *(const u32x4*)(lA + a_lane[mt] + t * 64 + ks * 32);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int t = 0; t < TERMS; ++t) bf[nt][t] = *(const u32x4*)(lB + b_lane[nt] + t * 64 + ks * 32);
            if (TERMS == 3) {
                OCCD_GNT(1, 1);
                OCCD_GNT(0, TERMS == 3 ? 2 : 0);
                OCCD_GNT(TERMS == 3 ? 2 : 0, 0);
                OCCD_GNT(0, 1);
                OCCD_GNT(1, 0);
            }
            OCCD_GNT(0, 0);
        }
    }
#undef OCCD_GNT
    float* const Cb = p.C + ((size_t)bz * gridDim.z + blockIdx.z) * p.sC;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + (wn * NT + nt) * 32 + li;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int mb = m0 + (wm * MT + mt) * 32 + 4 * h;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mb + (r & 3) + 8 * (r >> 2);
                if (n < p.N && m < p.M) Cb[(size_t)m * p.ldc + n] = acc[mt][nt][r];
            }
        }
    }
}

struct VariantG {
    int MT, NT, WM, WN;
    void (*kern[5])(const GemmP);     // [pre 0 / 1 / 2] with the split; [3] = float32 operands rounded to ONE bf16 term;
                                      // [4] = A from the f16x2 image, the two-term fp16 split
};
#define OCCD_VARIANT_G(MT, NT, WM, WN) \
    VariantG{MT, NT, WM, WN, {gemm_x3_kernel<MT, NT, WM, WN, 0>, gemm_x3_kernel<MT, NT, WM, WN, 1>, gemm_x3_kernel<MT, NT, WM, WN, 2>, \
                              gemm_x3_kernel<MT, NT, WM, WN, 0, 1>, gemm_x3_kernel<MT, NT, WM, WN, 1, 2>}}
const VariantG kVariantsG[] = {
    OCCD_VARIANT_G(2, 2, 4, 2),   // 0: 256 x 128, 512 threads
    OCCD_VARIANT_G(2, 2, 2, 2),   // 1: 128 x 128, 256 threads
    OCCD_VARIANT_G(2, 1, 2, 2),   // 2: 128 x 64
    OCCD_VARIANT_G(1, 1, 2, 2),   // 3: 64 x 64
    OCCD_VARIANT_G(2, 2, 1, 4),   // 4: 64 x 256 (few rows, many columns: project convolutions at high resolution, M = 48 ... 64)
};
constexpr int kNumVariantsG = sizeof(kVariantsG) / sizeof(kVariantsG[0]);

// role 0: the A operand (rows x K, k contiguous) -> [row tile 32][k16][term][lane][8]: lane = (row & 31) + 32 ((k & 15) >> 3)
// role 1: the B operand (K x cols, column contiguous) -> the same image with "row" = column
__global__ void gemm_x3_pack_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int rows, int K, long ld,
                                    int role, long in_stride, long out_stride, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = i & 7, lane = (i >> 3) & 63;
    long t = i >> 9;
    const int K16 = (K + 15) >> 4;
    const int k16 = t % K16;
    const int rt = t / K16;
    const int r = rt * 32 + (lane & 31), k = k16 * 16 + (lane >> 5) * 8 + j;
    const float* src = w + (size_t)blockIdx.y * in_stride;
    float v = 0.f;
    if (r < rows && k < K) v = role == 0 ? src[(size_t)r * ld + k] : src[(size_t)k * ld + r];
    const __bf16 hi = (__bf16)v;
    const float r1 = v - (float)hi;
    const __bf16 mid = (__bf16)r1;
    const __bf16 lo = (__bf16)(r1 - (float)mid);
    uint16_t* dst = out + (size_t)blockIdx.y * out_stride + ((size_t)(rt * K16 + k16) * 3) * 512 + lane * 8 + j;
    dst[0] = __builtin_bit_cast(uint16_t, hi);
    dst[512] = __builtin_bit_cast(uint16_t, mid);
    dst[1024] = __builtin_bit_cast(uint16_t, lo);
}

// The f16x2 image of an A operand: the fragment order above with two fp16 terms, [row tile 32][k16][hi, lo][lane][8], of
// w'[m][k] = 2^k[m] w[m][k] -- k[m] puts the row's max |w'| into [2^13, 2^14); an all-zero row keeps k = 0 -- followed by one
// float per row of the padded row tiles, fac[m] = 2^-(k[m] + kF2XExp): the scheme of occd_pack_weights_f16x2
// (csrc/conv3d_bf16.hip) and wino_pack_f16x2_kernel, per ROW of a GEMM.  One 64-thread block per row finds the scale; a row with
// a non-finite weight is marked with a NaN factor, which the entry point reads back.
__global__ void __launch_bounds__(64) gemm_f16x2_scale_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int rows,
                                                              int K, long ld, long in_stride, long out_stride, long img) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const float* src = w + (size_t)blockIdx.y * in_stride + (size_t)r * ld;
    float m = 0.f;
    int bad = 0;
    if (r < rows) {
        for (int k = lane; k < K; k += 64) {
            const float v = fabsf(src[k]);
            if (!(v <= 3.0e38f)) bad = 1;                  // Inf or NaN (fmaxf would drop it)
            m = fmaxf(m, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmaxf(m, __shfl_xor(m, o));
        bad |= __shfl_xor(bad, o);
    }
    if (lane != 0) return;
    int e = 0;
    const bool ok = m > 0.f && !bad;
    if (ok) frexpf(m, &e);                                 // m in [2^(e-1), 2^e)
    const int k = ok ? min(max(14 - e, -100), 100) : 0;
    float* fac = reinterpret_cast<float*>(out + (size_t)blockIdx.y * out_stride + img);
    fac[r] = bad ? __builtin_nanf("") : ldexpf(1.f, -(k + kF2XExp));
}

__global__ void gemm_f16x2_pack_kernel(const float* __restrict__ w, uint16_t* __restrict__ out, int rows, int K, long ld,
                                       long in_stride, long out_stride, long img) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= img / 2) return;
    const int j = i & 7, lane = (i >> 3) & 63;
    const long t = i >> 9;
    const int K16 = (K + 15) >> 4;
    const int k16 = t % K16;
    const int rt = t / K16;
    const int r = rt * 32 + (lane & 31), k = k16 * 16 + (lane >> 5) * 8 + j;
    uint16_t* const dst0 = out + (size_t)blockIdx.y * out_stride;
    const float* fac = reinterpret_cast<const float*>(dst0 + img);
    float v = 0.f;
    if (r < rows && k < K) v = w[(size_t)blockIdx.y * in_stride + (size_t)r * ld + k] * (ldexpf(1.f, -kF2XExp) / fac[r]);   // 2^k[m]: exact
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);
    uint16_t* dst = dst0 + ((size_t)(rt * K16 + k16) * 2) * 512 + lane * 8 + j;
    dst[0] = __builtin_bit_cast(uint16_t, hi);
    dst[512] = __builtin_bit_cast(uint16_t, lo);
}

// 16-bit elements of the f16x2 image in front of its factors
inline int64_t f16x2_image_elems(int32_t rows, int32_t K) { return (int64_t)((rows + 31) / 32) * ((K + 15) / 16) * 2 * 512; }

}  // namespace

extern "C" int64_t occd_gemm_f16x2_packed_elems(int32_t rows, int32_t K) {
    if (rows <= 0 || K <= 0) return OCCD_EINVAL;
    return f16x2_image_elems(rows, K) + (int64_t)((rows + 31) / 32) * 32 * 2;
}

extern "C" int occd_gemm_f16x2_pack(const float* w, void* out, int32_t rows, int32_t K, int64_t ld, int32_t batch,
                                    int64_t in_stride, void* stream) {
    if (!w || !out || rows <= 0 || K <= 0 || batch <= 0 || batch > 65535 || ld < K) return OCCD_EINVAL;
    if (reinterpret_cast<uintptr_t>(out) & 15) return OCCD_EINVAL;
    const int64_t per = occd_gemm_f16x2_packed_elems(rows, K), img = f16x2_image_elems(rows, K);
    const int rows_pad = (rows + 31) / 32 * 32;
    hipStream_t st = (hipStream_t)stream;
    {
        occd::ProfScope prof("gemm_f16x2_pack", st, 0.0, (double)per * 2 * batch);
        hipLaunchKernelGGL(gemm_f16x2_scale_kernel, dim3((unsigned)rows_pad, (unsigned)batch), dim3(64), 0, st, w, (uint16_t*)out,
                           rows, K, (long)ld, (long)in_stride, (long)per, (long)img);
        hipLaunchKernelGGL(gemm_f16x2_pack_kernel, dim3((unsigned)((img / 2 + 255) / 256), (unsigned)batch), dim3(256), 0, st, w,
                           (uint16_t*)out, rows, K, (long)ld, (long)in_stride, (long)per, (long)img);
        const int rc = occd::check_launch();
        if (rc != OCCD_OK) return rc;
    }
    // a non-finite weight has no power-of-two scale: read the factors back (packing is a set-up step, never part of a captured
    // forward) and refuse; the caller keeps the bf16x3 image of occd_gemm_x3_pack
    std::vector<float> host((size_t)rows_pad);
    for (int b = 0; b < batch; ++b) {
        const float* fac = reinterpret_cast<const float*>(static_cast<const uint16_t*>(out) + (size_t)b * per + img);
        if (hipMemcpyAsync(host.data(), fac, host.size() * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return OCCD_ELAUNCH;
        for (float f : host)
            if (f != f) return OCCD_EINVAL;
    }
    return OCCD_OK;
}

extern "C" int64_t occd_gemm_x3_packed_elems(int32_t rows, int32_t K) {
    if (rows <= 0 || K <= 0) return OCCD_EINVAL;
    return (int64_t)((rows + 31) / 32) * ((K + 15) / 16) * 3 * 512;
}

extern "C" int occd_gemm_x3_pack(const float* w, void* out, int32_t rows, int32_t K, int64_t ld, int32_t role, int32_t batch,
                                 int64_t in_stride, void* stream) {
    if (!w || !out || rows <= 0 || K <= 0 || role < 0 || role > 1 || batch <= 0 || batch > 65535) return OCCD_EINVAL;
    if (ld < (role == 0 ? K : rows)) return OCCD_EINVAL;
    const int64_t per = occd_gemm_x3_packed_elems(rows, K);
    const long total = per / 3;
    occd::ProfScope prof("gemm_x3_pack", (hipStream_t)stream, 0.0, (double)per * 2 * batch);
    hipLaunchKernelGGL(gemm_x3_pack_kernel, dim3((unsigned)((total + 255) / 256), (unsigned)batch), dim3(256), 0,
                       (hipStream_t)stream, w, (uint16_t*)out, rows, K, (long)ld, role, (long)in_stride, (long)per, total);
    return occd::check_launch();
}

// The hint-0 decision of occd_gemm_f32x3 (and what a forcing hint turns it into), from shapes alone: which kernel family
// (OCCD_GEMM_KERNEL_*) and which variant of it -- PANEL: the panel width in 32-column units (1 / 2); TILE, WS, KSPLIT: the
// index into kVariantsG.  pre: occd_gemm_args.pre; plain: no res, no scale_k, no act_a, no bias_n.  OCCD_EINVAL for a shape
// or a hint / pre combination occd_gemm_f32x3 rejects.  Host code only: occd_gemm_f32x3 launches what this returns, and
// occd_gemm_f32x3_route answers callers that pack weight images per route (occdepth_amd/hip.py).
static int gemm_route(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t pre, int32_t plain, int32_t tile_hint,
                      int32_t* kernel, int32_t* variant) {
    if (M <= 0 || N < 4 || K <= 0 || (K & 7) || batch <= 0 || batch > 65535) return OCCD_EINVAL;
    if (pre < 0 || pre > OCCD_GEMM_PRE_F16X2 || tile_hint < 0 || tile_hint > kNumVariantsG + 3) return OCCD_EINVAL;
    const bool img_a = pre == 1 || pre == OCCD_GEMM_PRE_F16X2;
    {
        // K16p: pre-split A, the whole-K panel of 32 / 64 B columns fits LDS, plain epilogue.  hint 8 forces it, hint 0 picks it
        // for matrices of >= 256 rows -- one row tile for each of the 8 waves (OCCD_GEMM_PANEL=0 keeps the barrier-phased
        // PRE = 1 kernel for A/B)
        static const bool panel_off = !occd::env_flag("OCCD_GEMM_PANEL", true);
        const int KP = ((K + 15) / 16) * 16;
        const bool fits1 = img_a && plain && (size_t)KP * panel_row_bytes(1) <= 160 * 1024;      // K <= 848
        const bool fits2 = img_a && plain && (size_t)KP * panel_row_bytes(2) <= 160 * 1024;      // K <= 352
        if (tile_hint == kNumVariantsG + 3 && !fits1) return OCCD_EINVAL;
        // (hint 0, K > 352 -- the 32-column form only: just the few-pixel launches of the 1/16 and 1/32 stages, where it leads by
        //  ~15 %; the 1/4-level tap GEMM, 2880 x 7191 x 640, measured 0.45 ms on it against K16's 0.35)
        const long small_launch = (long)((N + 63) / 64) * batch * (((M + 31) / 32 + 7) / 8);
        const bool auto_ok = tile_hint == 0 && !panel_off && M >= 256 && (fits2 || small_launch <= 512);
        if (fits1 && (tile_hint == kNumVariantsG + 3 || auto_ok)) {
            // panel width: 64 columns while two workgroups fit a CU's LDS with them (K <= 176), else 32 (measured, kernel trace,
            // profiles/r05_gemm_panel.txt: tap 1/2 (K = 320) 332 against 362 us, 224 -> 1344 on 1848 pixels 22 against 27 us; the
            // 64-column form ahead by 3 ... 10 % on K = 48 ... 160): a second resident workgroup stages its panel under the
            // first one's MFMAs, which is worth more than half the weight-fragment traffic
            int nt = (fits2 && (size_t)KP * panel_row_bytes(2) <= 80 * 1024) ? 2 : 1;
            static const int dev_nt = getenv("OCCD_GEMM_PANEL_NT") ? atoi(getenv("OCCD_GEMM_PANEL_NT")) : 0;     // (development A/B)
            if ((dev_nt == 1 || dev_nt == 2) && (dev_nt == 1 || fits2)) nt = dev_nt;
            *kernel = OCCD_GEMM_KERNEL_PANEL;
            *variant = nt;
            return OCCD_OK;
        }
    }
    int pick = tile_hint - 1;
    if (tile_hint == kNumVariantsG + 1) {
        if (pre != 0) return OCCD_EINVAL;
        pick = 0;
    }
    if (tile_hint == kNumVariantsG + 2) {
        if (pre != 0) return OCCD_EINVAL;
        pick = 3;
    }
    if (pick < 0) {
        // Long K (>= 1024: tap GEMMs, Winograd-domain products): the largest tile that still leaves >= 160 workgroups
        // (measured, profiles/r04_gemm_x3_v3_ws.txt: the large tiles win down to ~0.6 workgroups per CU).  Short K (the MBConv
        // expand convolutions, 32 ... 640 input channels = 1 ... 20 k-steps): a workgroup is mostly prologue + epilogue and only
        // several resident workgroups per CU hide it -- 64 x 64 tiles unless the problem is so large that even 256 x 128 tiles
        // give 8 workgroups per CU (profiles/r04_gemm_x3_v5_shortk.txt: 48 -> 288 on 28365 pixels 54 -> 34 us, 384 -> 2304 on
        // 468 pixels 27 -> 23 us; the tap GEMMs of the 1/1 and 1/2 levels, K = 160 / 320, keep 256 x 128); in between
        // (K = 512 ... 1023) the largest tile with >= 320 workgroups.  A matrix of <= 64 rows (project convolutions of the
        // high-resolution stages in training: M = 32 ... 64, N = 10^4 ... 10^5 pixels) takes the 64-row tiles instead of
        // wasting 3/4 of a 256-row one.
        auto wgs_of = [&](int i) {
            const VariantG& v = kVariantsG[i];
            const long tm = v.MT * v.WM * 32, tn = v.NT * v.WN * 32;
            return ((M + tm - 1) / tm) * ((N + tn - 1) / tn) * batch;
        };
        if (M <= 64) {
            // (short K: 64 x 64 again -- 288 -> 48 on 2 x 28365 pixels 30 us against 42 with 64 x 256 tiles)
            pick = (K >= 512 && (long)((N + 255) / 256) * batch >= 160) ? 4 : 3;
        } else if (K < 512) {
            pick = wgs_of(0) >= 2048 ? 0 : 3;
        } else {
            const long need = K < 1024 ? 320 : 160;
            pick = 3;
            for (int i = 0; i < 4; ++i)
                if (wgs_of(i) >= need) { pick = i; break; }
        }
    }
    // the wave-specialised 256 x 128 kernel takes the launches the 256 x 128 tile would (float32 operands): hint 6 forces it,
    // hint 0 picks it (OCCD_GEMM_WS=0 in the environment keeps the barrier-phased kernels for A/B)
    static const bool ws_off = !occd::env_flag("OCCD_GEMM_WS", true);
    // measured (profiles/r04_gemm_x3_v4_fast.txt): with the tail-free fast path the barrier-phased kernel leads everywhere but on
    // the longest K (tap GEMM of the 1/16 level, K = 2560: 0.438 against 0.462 ms); K16w keeps that launch
    const bool ws = pre == 0 && plain && (tile_hint == kNumVariantsG + 1 || (tile_hint == 0 && pick == 0 && !ws_off && K >= 2048));
    // in-workgroup split-K (64 x 64 tile, 4 K groups = 16 waves) when the 64 x 64 tiling leaves CUs without a workgroup and K is
    // long: the project convolutions of the 1/16 and 1/32 stages (tile_hint 7 forces it; OCCD_GEMM_KS=0 disables it for A/B)
    static const bool ks_off = !occd::env_flag("OCCD_GEMM_KS", true);
    const long wgs64 = (long)((M + 63) / 64) * ((N + 63) / 64) * batch;
    const bool ksplit = pre == 0 && !ws && (tile_hint == kNumVariantsG + 2 ||
                                            (tile_hint == 0 && pick == 3 && !ks_off && K >= 768 && wgs64 <= 320));
    *kernel = ws ? OCCD_GEMM_KERNEL_WS : ksplit ? OCCD_GEMM_KERNEL_KSPLIT : OCCD_GEMM_KERNEL_TILE;
    *variant = pick;
    return OCCD_OK;
}

extern "C" int occd_gemm_f32x3_route(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t pre, int32_t plain, int32_t tile_hint,
                                     int32_t* kernel, int32_t* variant) {
    if (!kernel || !variant) return OCCD_EINVAL;
    return gemm_route(M, N, K, batch, pre, plain, tile_hint, kernel, variant);
}

// a->tile_hint: 0 = pick (see below), 1 .. 5 = force a tile variant, 6 = force K16w, 7 = force the 64 x 64 split-K form,
// 8 = force K16p (pre = 1, K <= 848, no res / scale_k).
// a->pre: 0 = A and B float32; 1 = a->A is the role-0 image of occd_gemm_x3_pack (lda ignored, stride_a = bf16 elements
// between batch items, 0 = shared); 2 = a->B is the role-1 image (ldb ignored, stride_b likewise); OCCD_GEMM_PRE_F16X2 (4) = a->A
// is the image of occd_gemm_f16x2_pack (stride_a = 16-bit elements, factors included): the two-term fp16 split on the tile
// variants and K16p (hints 0 .. 5 and 8; no act_a / bias_n).
extern "C" int occd_gemm_f32x3(const occd_gemm_args* a, void* stream) {
    if (!a || !a->A || !a->B || !a->C) return OCCD_EINVAL;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0 || a->batch > 65535) return OCCD_EINVAL;
    if (a->pre < 0 || a->pre > OCCD_GEMM_PRE_F16X2) return OCCD_EINVAL;      // 3: float32 operands, plain bf16 arithmetic (one term)
    const bool f16x2 = a->pre == OCCD_GEMM_PRE_F16X2, img_a = a->pre == 1 || f16x2;
    if (f16x2 && (a->act_a != 0 || a->bias_n != nullptr || a->tile_hint == kNumVariantsG + 1 || a->tile_hint == kNumVariantsG + 2))
        return OCCD_EINVAL;
    if ((a->K & 7) || a->ldc < a->N || a->N < 4) return OCCD_EINVAL;
    if (!img_a && ((a->lda & 3) || a->lda < a->K || (reinterpret_cast<uintptr_t>(a->A) & 15) || (a->stride_a & 3)))
        return OCCD_EINVAL;
    if (a->pre != 2 && (a->ldb < a->N || (reinterpret_cast<uintptr_t>(a->B) & 3))) return OCCD_EINVAL;
    if (img_a && ((reinterpret_cast<uintptr_t>(a->A) & 15) || (a->stride_a & 7))) return OCCD_EINVAL;
    if (a->pre == 2 && ((reinterpret_cast<uintptr_t>(a->B) & 15) || (a->stride_b & 7))) return OCCD_EINVAL;
    if (reinterpret_cast<uintptr_t>(a->C) & 3) return OCCD_EINVAL;
    if (a->act < 0 || a->act > 2 || a->tile_hint < 0 || a->tile_hint > kNumVariantsG + 3) return OCCD_EINVAL;
    if (a->res != nullptr && (reinterpret_cast<uintptr_t>(a->res) & 3)) return OCCD_EINVAL;
    if (a->bias_n != nullptr && ((reinterpret_cast<uintptr_t>(a->bias_n) & 3) || a->stride_bias_n < 0 ||
                                 a->tile_hint == kNumVariantsG + 1 || a->tile_hint == kNumVariantsG + 3))
        return OCCD_EINVAL;                              // (the wave-specialised and the panel kernels have no column bias)
    if ((a->res != nullptr || a->scale_k != nullptr) && (a->tile_hint == kNumVariantsG + 1 || a->pre == 2)) return OCCD_EINVAL;
    if (a->act_a != 0 && (a->act_a != 1 || img_a || a->pre == 3 || a->tile_hint == kNumVariantsG + 1)) return OCCD_EINVAL;
    const bool plain = a->res == nullptr && a->scale_k == nullptr && a->act_a == 0 && a->bias_n == nullptr;
    int32_t route = 0, pick = 0;
    if (gemm_route(a->M, a->N, a->K, a->batch, a->pre, plain, a->tile_hint, &route, &pick) != OCCD_OK) return OCCD_EINVAL;
    if (route == OCCD_GEMM_KERNEL_PANEL) {
        const int nt = pick, KP = ((a->K + 15) / 16) * 16;
        GemmP p;
        p.A = a->A; p.B = a->B; p.C = a->C; p.bias = a->bias; p.res = nullptr; p.kscale = nullptr;
        p.M = a->M; p.N = a->N; p.K = a->K;
        p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc; p.sA = a->stride_a / 8; p.sB = a->stride_b; p.sC = a->stride_c;
        p.act = a->act; p.slope = a->slope; p.act_a = 0; p.n_fast = 1;
        const int tiles = (a->M + 31) / 32, r8 = (tiles + 7) / 8;
        if (f16x2) {
            p.fac = reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(a->A) + f16x2_image_elems(a->M, a->K));
            p.s_fac = a->stride_a / 2;
        }
        p.ntiles = (a->N + 32 * nt - 1) / (32 * nt);
        const long panels = (long)p.ntiles * a->batch;
        // row ranges: ranges of 8 row tiles (one per wave) while that gives at most ~4 workgroups per CU; a large launch
        // walks all its row tiles in every workgroup (the panel is staged once), cut only as far as 256 CUs need it
        long ranges = panels * r8 <= 1024 ? r8 : panels >= 256 ? 1 : 256 / panels;
        if (ranges > r8) ranges = r8;
        if (ranges < 1) ranges = 1;
        static const int dev_ranges = getenv("OCCD_GEMM_PANEL_RANGES") ? atoi(getenv("OCCD_GEMM_PANEL_RANGES")) : 0;
        if (dev_ranges >= 1 && dev_ranges <= tiles) ranges = dev_ranges;
        p.mr_tiles = (int)((tiles + ranges - 1) / ranges);
        p.mtiles = (tiles + p.mr_tiles - 1) / p.mr_tiles;
        // row tiles per wave and round (MT): 1.  Measured (profiles/r05_gemm_panel.txt): 2 / 3 tiles per wave halve / third
        // the LDS fragment reads but lose on every launch of the frame (tap 1/1 460 -> 471 / 487 us, 48 -> 288 on 28365
        // pixels 29 -> 37 / 45 us): several short rounds per wave overlap one wave's stores with the other's MFMAs; raising
        // the priority of one wave per SIMD to force that alternation changed nothing.
        const long nwg = (long)p.mtiles * p.ntiles;
        if (nwg >= (1L << 31)) return OCCD_EINVAL;
        p.nwg = (unsigned)nwg;
        // weight fragments ONE step ahead; two on the 32-column form with a long K (K >= 512: 42.8 -> 40.0 us, 40.2 -> 37.8).
        // Measured with the branch-free loop below, i.e. with the loads really in flight (ISA: vmcnt(10) ... vmcnt(1)):
        // deeper is slower on every other launch (tap 1/1 369 -> 384 / 382 / 412 us at 2 / 4 / 6 steps, 48 -> 288 27 -> 31 -> 41)
        // -- tools/panel_timeline.cpp shows a 16-k step at ~700 cycles (32 columns) / ~950 (64) whatever the depth: the two
        // waves of a SIMD keep the matrix pipe 55 - 70 % busy INSIDE the loop; the launch-level 22 - 35 % is prologue (kernel
        // arguments + panel staging: 7k cycles of a 29k-cycle workgroup at 384 -> 2304 on 468 pixels), epilogue and dispatch.
        // f16x2: the same widths and depths (the routing limits of gemm_route are those of the three-term rows, so that a launch
        // takes the same route under either split; the 64-column row of 320 B would leave two workgroups per CU up to K = 256 --
        // not measured, K <= 176 kept)
        void (*kern)(const GemmP) = nt == 2 ? gemm_x3_panel_kernel<1, 2, 1> : a->K >= 512 ? gemm_x3_panel_kernel<1, 1, 2> : gemm_x3_panel_kernel<1, 1, 1>;
        if (f16x2) kern = nt == 2 ? gemm_x3_panel_kernel<1, 2, 1, 2> : a->K >= 512 ? gemm_x3_panel_kernel<1, 1, 2, 2> : gemm_x3_panel_kernel<1, 1, 1, 2>;
        const size_t plds = (size_t)KP * panel_row_bytes(nt, f16x2 ? 2 : 3);
        if (plds > 64 * 1024 && occd::ensure_big_lds(reinterpret_cast<const void*>(kern)) != OCCD_OK) return OCCD_ELAUNCH;
        const double flops = 2.0 * a->M * a->N * a->K * a->batch;
        const double bytes = 4.0 * ((double)a->M * a->K * (a->stride_a != 0 ? a->batch : 1) + ((double)a->K + a->M) * a->N * a->batch);
        occd::ProfScope prof("gemm_f32x3_panel", (hipStream_t)stream, flops, bytes);
        hipLaunchKernelGGL(kern, dim3((unsigned)nwg, (unsigned)a->batch), dim3(512), plds, (hipStream_t)stream, p);
        return occd::check_launch();
    }
    const bool ws = route == OCCD_GEMM_KERNEL_WS, ksplit = route == OCCD_GEMM_KERNEL_KSPLIT;
    const VariantG& v = kVariantsG[pick];
    const int TM = v.MT * v.WM * 32, TN = v.NT * v.WN * 32;
    GemmP p;
    p.A = a->A; p.B = a->B; p.C = a->C; p.bias = a->bias; p.res = a->res; p.kscale = a->scale_k;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc; p.sA = a->stride_a; p.sB = a->stride_b; p.sC = a->stride_c;
    if (img_a) p.sA = a->stride_a / 8;              // 16-bit elements -> u32x4 records
    if (f16x2) {
        p.fac = reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(a->A) + f16x2_image_elems(a->M, a->K));
        p.s_fac = a->stride_a / 2;
    }
    if (a->pre == 2) p.sB = a->stride_b / 8;
    p.act = a->act; p.slope = a->slope; p.act_a = a->act_a;
    p.bias_n = a->bias_n; p.s_bias_n = a->stride_bias_n;
    p.mtiles = (a->M + TM - 1) / TM;
    p.ntiles = (a->N + TN - 1) / TN;
    // the tile of the LARGER operand is the one worth fetching once per L2: iterate over the other dimension fastest
    p.n_fast = (double)a->M * a->K * (a->stride_a != 0 ? a->batch : 1) >= (double)a->K * a->N * a->batch ? 1 : 0;
    const long nwg = (long)p.mtiles * p.ntiles;
    if (nwg >= (1L << 31)) return OCCD_EINVAL;
    p.nwg = (unsigned)nwg;
    constexpr int kKS = 4;
    const size_t lds = ws ? (size_t)2 * kWsStage
                          : ((img_a ? 0 : (size_t)TM * kARow) + (a->pre == 2 ? 0 : (size_t)(f16x2 ? 2 : 3) * 32 * (TN * 2 + 64))) * (ksplit ? kKS : 1);
    void (*kern)(const GemmP) = ws ? gemm_x3_ws_kernel<0> : ksplit ? gemm_x3_kernel<1, 1, 2, 2, 0, 3, kKS> : v.kern[a->pre];
#ifdef OCCD_GEMM_DEV_VARIANTS
    if (ws && getenv("OCCD_GEMM_DBG") != nullptr)
        kern = getenv("OCCD_GEMM_DBG")[0] == '1' ? gemm_x3_ws_kernel<1> : getenv("OCCD_GEMM_DBG")[0] == '2' ? gemm_x3_ws_kernel<2> :
               getenv("OCCD_GEMM_DBG")[0] == '3' ? gemm_x3_ws_kernel<3> : getenv("OCCD_GEMM_DBG")[0] == '4' ? gemm_x3_ws_kernel<4> :
               getenv("OCCD_GEMM_DBG")[0] == '5' ? gemm_x3_ws_kernel<5> : kern;
#endif
    if (lds > 64 * 1024 && occd::ensure_big_lds(reinterpret_cast<const void*>(kern)) != OCCD_OK) return OCCD_ELAUNCH;
    const double flops = 2.0 * a->M * a->N * a->K * a->batch;
    const double bytes = 4.0 * ((double)a->M * a->K * (a->stride_a != 0 ? a->batch : 1) + ((double)a->K + a->M) * a->N * a->batch);
    occd::ProfScope prof(ws ? "gemm_f32x3_ws" : a->pre == 0 ? "gemm_f32x3" : img_a ? "gemm_f32x3_preA" : a->pre == 2 ? "gemm_f32x3_preB" : "gemm_bf16", (hipStream_t)stream, flops, bytes);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg, (unsigned)a->batch), dim3(ws ? 512 : v.WM * v.WN * 64 * (ksplit ? kKS : 1)), lds,
                       (hipStream_t)stream, p);
    return occd::check_launch();
}

// K21 (see gemm_x3_panel_splitk_kernel): a->pre must be 1 (A = the role-0 image of occd_gemm_x3_pack) or OCCD_GEMM_PRE_F16X2
// (the image of occd_gemm_f16x2_pack), B float32 with n
// contiguous, optional bias / act / res / scale_k as occd_gemm_f32x3.  `nz` K chunks of `k16_per_z` 16-k steps each
// (occd_gemm_f32x3_splitk_plan proposes them; k16_per_z * 192 B <= 160 KB of LDS, two workgroups per CU up to 26 steps),
// `row_ranges` >= 1 row ranges per panel, workspace: >= batch * nz * M * round_up(N, 32) floats.
extern "C" int occd_gemm_f32x3_splitk_plan(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t* k16_per_z, int32_t* nz,
                                           int32_t* row_ranges, int64_t* workspace_floats) {
    if (M <= 0 || N < 4 || K <= 0 || (K & 7) || batch <= 0 || !k16_per_z || !nz || !row_ranges || !workspace_floats) return OCCD_EINVAL;
    const int K16tot = (K + 15) / 16, tiles = (M + 31) / 32;
    const long panels = (long)((N + 31) / 32) * batch;
    // Measured on the five project-convolution shapes of config 2 (tools/bench_splitk.py, profiles/r06_gemm_splitk.txt): the best
    // plans all have ~240 workgroups -- ONE per CU -- with chunks as long as that allows (fewer chunks = less workspace traffic
    // for the second launch: 2304 -> 384 on 2 x 468 pixels 21.6 us with 4 chunks x 2 row ranges, 23.3 with 8 x 1, 30.9 with 18 x
    // 1); a chunk may use the whole LDS (<= 52 steps = 160 KB).  Row ranges: all row tiles in one workgroup (the chunk is
    // staged once) unless the matrix has 12 ... 16 row tiles -- then two ranges of 6 ... 8 tiles (one per wave) and half the chunks.
    // (never more workgroups than CUs: 9 chunks x 30 panels = 270 workgroups measured 60 us where 8 x 30 = 240 take 41 -- the
    //  chunks are long enough to hold a CU's LDS alone, so 14 stragglers are a second round)
    int z = (int)(256 / panels);
    if (z < 1) z = 1;
    int rr = 1;
    if (tiles >= 12 && tiles <= 16 && z >= 8) { z /= 2; rr = 2; }
    if (z > K16tot / 4) z = K16tot / 4 > 0 ? K16tot / 4 : 1;     // (at least 4 steps per chunk)
    if (z < (K16tot + 51) / 52) z = (K16tot + 51) / 52;
    int per = (K16tot + z - 1) / z;
    z = (K16tot + per - 1) / per;
    *k16_per_z = per; *nz = z; *row_ranges = rr;
    *workspace_floats = (int64_t)batch * z * M * (((int64_t)N + 31) / 32 * 32);
    return OCCD_OK;
}

extern "C" int occd_gemm_f32x3_splitk(const occd_gemm_args* a, int32_t k16_per_z, int32_t nz, int32_t row_ranges,
                                      float* workspace, int64_t workspace_floats, void* stream) {
    if (!a || !a->A || !a->B || !a->C || !workspace) return OCCD_EINVAL;
    if (a->M <= 0 || a->N < 4 || a->K <= 0 || (a->K & 7) || a->batch <= 0 || a->batch > 65535) return OCCD_EINVAL;
    const bool f16x2 = a->pre == OCCD_GEMM_PRE_F16X2;
    if ((a->pre != 1 && !f16x2) || a->act_a != 0 || a->act < 0 || a->act > 2 || a->ldc < a->N || a->ldb < a->N || a->bias_n != nullptr) return OCCD_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a->A) & 15) || (a->stride_a & 7) || (reinterpret_cast<uintptr_t>(a->B) & 3) ||
        (reinterpret_cast<uintptr_t>(a->C) & 3) || (reinterpret_cast<uintptr_t>(workspace) & 127))
        return OCCD_EINVAL;
    if (a->res != nullptr && (reinterpret_cast<uintptr_t>(a->res) & 3)) return OCCD_EINVAL;
    const int K16tot = (a->K + 15) / 16, tiles = (a->M + 31) / 32;
    if (k16_per_z < 1 || nz < 1 || nz > 65535 || row_ranges < 1 || row_ranges > tiles) return OCCD_EINVAL;
    if ((long)(nz - 1) * k16_per_z >= K16tot || (long)nz * k16_per_z < K16tot) return OCCD_EINVAL;      // every chunk non-empty, all of K covered
    const size_t lds = (size_t)k16_per_z * 16 * panel_row_bytes(1);
    if (lds > 160 * 1024) return OCCD_EINVAL;
    const long ld_ws = ((long)a->N + 31) / 32 * 32;
    if (workspace_floats < (int64_t)a->batch * nz * a->M * ld_ws) return OCCD_EINVAL;
    GemmSKP q;
    GemmP& p = q.g;
    p.A = a->A; p.B = a->B; p.C = a->C; p.bias = nullptr; p.res = nullptr; p.kscale = a->scale_k;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc; p.sA = a->stride_a / 8; p.sB = a->stride_b; p.sC = a->stride_c;
    p.act = 0; p.slope = 0.f; p.act_a = 0; p.n_fast = 1;
    p.ntiles = (a->N + 31) / 32;
    p.mr_tiles = (tiles + row_ranges - 1) / row_ranges;
    p.mtiles = (tiles + p.mr_tiles - 1) / p.mr_tiles;
    const long nwg = (long)p.mtiles * p.ntiles;
    if (nwg >= (1L << 31)) return OCCD_EINVAL;
    p.nwg = (unsigned)nwg;
    q.k16_per_z = k16_per_z;
    q.ws = workspace;
    q.ld_ws = ld_ws;
    q.z_stride = (long)a->M * ld_ws;
    q.b_stride = (long)nz * q.z_stride;
    void (*kern)(const GemmSKP) = k16_per_z >= 16 ? gemm_x3_panel_splitk_kernel<1, 2> : gemm_x3_panel_splitk_kernel<1, 1>;
    if (f16x2) kern = k16_per_z >= 16 ? gemm_x3_panel_splitk_kernel<1, 2, 2> : gemm_x3_panel_splitk_kernel<1, 1, 2>;
    // (the 32-column row of the f16x2 panel is 192 B as well: the same LDS bound, the same plan)
    const float* const fac = f16x2 ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(a->A) + f16x2_image_elems(a->M, a->K))
                                   : nullptr;
    if (lds > 64 * 1024 && occd::ensure_big_lds(reinterpret_cast<const void*>(kern)) != OCCD_OK) return OCCD_ELAUNCH;
    hipStream_t st = (hipStream_t)stream;
    const double flops = 2.0 * a->M * a->N * a->K * a->batch;
    const double bytes = 4.0 * ((double)a->M * a->K * (a->stride_a != 0 ? a->batch : 1) + ((double)a->K + a->M) * a->N * a->batch);
    occd::ProfScope prof("gemm_f32x3_splitk", st, flops, bytes);
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg, (unsigned)a->batch, (unsigned)nz), dim3(512), lds, st, q);
    const int vec_ok = ((a->ldc & 3) == 0 && (a->stride_c & 3) == 0 && (reinterpret_cast<uintptr_t>(a->C) & 15) == 0 &&
                        (a->res == nullptr || (reinterpret_cast<uintptr_t>(a->res) & 15) == 0)) ? 1 : 0;
    const long items = (long)a->M * ((a->N + 3) / 4);
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((items + 255) / 256), (unsigned)a->batch), dim3(256), 0, st,
                       (const float*)workspace, a->C, a->bias, a->res, a->M, a->N, nz, ld_ws, q.z_stride, q.b_stride,
                       (long)a->ldc, (long)a->stride_c, a->act, a->slope, vec_ok, fac);
    return occd::check_launch();
}

// K16t: C[b][z] = A[b] . B[b]^T over the z-th K range, with both operands k-contiguous (lda, ldb >= K; any dword alignment;
// any K >= 1): the weight gradient of a pointwise convolution, dW = gy (Cout x HW) . x^T.  a->act carries the number of
// K splits (>= 1; occd_gemm_f32x3_nt_splits proposes one): C holds batch x splits partial matrices, stride_c elements apart
// (batch-major), which the caller sums.  bias / pre must be NULL / 0.
extern "C" int32_t occd_gemm_f32x3_nt_splits(int32_t M, int32_t N, int32_t K, int32_t batch) {
    if (M <= 0 || N <= 0 || K <= 0 || batch <= 0) return OCCD_EINVAL;
    const long tiles128 = (long)((M + 127) / 128) * ((N + 127) / 128) * batch;
    const bool small = tiles128 < 32;
    const long tiles = small ? (long)((M + 63) / 64) * ((N + 63) / 64) * batch : tiles128;
    const int steps = (K + 31) / 32;
    long want = (768 + tiles - 1) / tiles;          // ~3 workgroups per CU
    if (want > steps / 4) want = steps / 4;          // at least 4 K steps (128 k) per split
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    return (int32_t)want;
}

extern "C" int occd_gemm_f32x3_nt(const occd_gemm_args* a, void* stream) {
    if (!a || !a->A || !a->B || !a->C) return OCCD_EINVAL;
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0 || a->batch > 65535) return OCCD_EINVAL;
    if (a->lda < a->K || a->ldb < a->K || a->ldc < a->N || (a->pre != 0 && a->pre != 3) || a->bias != nullptr || a->res != nullptr ||
        a->scale_k != nullptr || a->bias_n != nullptr)
        return OCCD_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a->A) & 3) || (reinterpret_cast<uintptr_t>(a->B) & 3) || (reinterpret_cast<uintptr_t>(a->C) & 3))
        return OCCD_EINVAL;
    const int steps = (a->K + 31) / 32;
    const int splits = a->act;
    if (a->tile_hint < 0 || a->tile_hint > 2 || splits < 1 || splits > 65535 || splits > steps) return OCCD_EINVAL;
    // 128 x 128 tiles unless that leaves too few of them (weight matrices are small: M x N = Cout x Cin)
    const long wg128 = (long)((a->M + 127) / 128) * ((a->N + 127) / 128) * a->batch;
    const bool small = a->tile_hint == 2 || (a->tile_hint == 0 && wg128 < 32);
    const int TM = small ? 64 : 128, TN = small ? 64 : 128;
    GemmP p;
    p.A = a->A; p.B = a->B; p.C = a->C; p.bias = nullptr; p.res = nullptr; p.kscale = nullptr;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc; p.sA = a->stride_a; p.sB = a->stride_b; p.sC = a->stride_c;
    p.act = (steps + splits - 1) / splits;            // (the kernel reads p.act as "32-k steps per split")
    p.slope = 0.f;
    p.mtiles = (a->M + TM - 1) / TM;
    p.ntiles = (a->N + TN - 1) / TN;
    p.n_fast = 0;
    const long nwg = (long)p.mtiles * p.ntiles;
    if (nwg >= (1L << 31)) return OCCD_EINVAL;
    p.nwg = (unsigned)nwg;
    const int zsplits = (steps + p.act - 1) / p.act;  // splits that own at least one step
    if (zsplits != splits) return OCCD_EINVAL;        // (the caller sized C for `splits` partials: every one must be written)
    const size_t lds = (size_t)(TM + TN) * kARow;
    void (*kern)(const GemmP) = a->pre == 3 ? (small ? gemm_x3_nt_kernel<1, 1, 2, 2, 1> : gemm_x3_nt_kernel<2, 2, 2, 2, 1>)
                                            : (small ? gemm_x3_nt_kernel<1, 1, 2, 2> : gemm_x3_nt_kernel<2, 2, 2, 2>);
    if (lds > 64 * 1024 && occd::ensure_big_lds(reinterpret_cast<const void*>(kern)) != OCCD_OK) return OCCD_ELAUNCH;
    const double flops = 2.0 * a->M * a->N * a->K * a->batch;
    occd::ProfScope prof(a->pre == 3 ? "gemm_bf16_nt" : "gemm_f32x3_nt", (hipStream_t)stream, flops, 4.0 * a->batch * ((double)(a->M + a->N) * a->K + (double)a->M * a->N * splits));
    hipLaunchKernelGGL(kern, dim3((unsigned)nwg, (unsigned)a->batch, (unsigned)splits), dim3(256), lds, (hipStream_t)stream, p);
    return occd::check_launch();
}
