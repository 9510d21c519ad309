// K10 -- fused Winograd F(2x2, 3x3) convolution on the CDNA4 fp32 matrix pipe.
//
//   y = act( conv3x3(x, g * scale[co], stride 1, pad 1) + shift[co] ) (+ res)       x, y, res: NCHW float32
//
// Per 2x2 output tile with 4x4 input patch d:   Y = A^T [ sum_cin U_cin (.) V_cin ] A,   U = G g G^T,  V = B^T d B.
// The 16 positions xi of the Winograd domain are 16 independent GEMMs over cin: 2.25x fewer multiplies than the direct
// form.  csrc/wino2d.hip runs them unfused (V and M round-trip through HBM: 4x the input and 4x the output bytes),
// which only pays where tiles are few; this kernel keeps everything on chip:
//   * a workgroup (8 waves) owns 128 tiles x 32 couts; a PAIR of waves owns 32 tiles x 32 couts and all 16 xi, 8 each
//     (8 accumulator tiles of v_mfma_f32_32x32x2_f32 = 128 AGPRs per wave, two waves per SIMD); the output transform
//     needs the 16 xi of one (tile, cout) together, so the pair swaps half of its accumulators through LDS once, after
//     the K loop -- M never exists in memory;
//   * cin is walked in chunks of 8: the chunk's input patch (8 x PR x PC, zero padded = the convolution's padding) is
//     staged into LDS by LDS-DMA (double buffered, one barrier per chunk, chunk c+1 lands under the MFMAs of chunk c);
//   * V never exists in memory either: a lane is the MFMA column of ONE tile and of 4 of the chunk's 8 cins (the K
//     index is permuted so lane half h owns cins 4h..4h+3, as in K2), so it reads exactly its own 4x4 patches from
//     LDS (ds_read_b64, conflict-free row stride), transforms them on the VALU (32 adds per patch) and feeds the 64
//     resulting values to the MFMAs as B operands; no V staging, no LDS writes besides the raw patch;
//   * U (BatchNorm scale folded in) is pre-packed in A-fragment order [chunk][4 q + 2 h + part][cout/32][lane][4 xi] (L2 resident,
//     <= 1 MB for the high-resolution decoder levels) and also arrives by LDS-DMA, 16 KB per chunk, read back as
//     ds_read_b128 fragments by all four waves;
//   * epilogue: A^T m A in registers (24 adds per (tile, cout)), + shift, activation, optional residual, NCHW
//     stores of 2-pixel pairs (16 consecutive lanes = 16 consecutive tiles = 128 contiguous bytes).
// MFMA work per launch: 2 * 16 * tiles * Cin8 * Cout32 FLOP (= direct FLOPs / 2.25 up to channel padding);
// algorithmic HBM bytes: 4 * (B Cin H W + B Cout H W) + the packed U.
//
// Reference semantics replaced: nn.Conv2d(k=3, s=1, p=1) + BatchNorm2d (eval) + LeakyReLU of
// occdepth/models/unet2d.py:24-46 (UpSampleBN), and the 3x3 convolutions of DepthNet / BasicBlock
// (occdepth/models/flosp_depth/flosp_depth.py:201-257).
#include <atomic>
#include <type_traits>
#include <vector>
#include "device.h"

namespace {

struct WinoP {
    const float* x;
    const float* upk;
    const float* shift;
    const float* res;
    float* y;
    int B, Cin, Cout, H, W;
    int chunks, nblk, wg_ty, wg_tx, nwg;
    int act, res_first;
    float slope;
};

// The pair exchange and the epilogue of K10 and K10h (FAC: K10h's per-cout factor in front of the shift).
// ---------------- pair exchange: wave half h finishes the cout registers r in [8h, 8h + 8) and needs the partner's 8 xi for
// them.  NPART = 1: one exchange of all 8 registers, xchg[pair][writer half][k * 8 + (r & 7)][lane] (128 KB; the staging
// buffers are dead: the caller's last barrier).  NPART = 2 (the persistent K10h): two exchanges of 4 registers each through
// xchg[pair][writer half][k * 4 + (r & 3)][lane] (64 KB), so that the buffer fits BEHIND the first patch buffer, which the
// next item's first patch is landing in meanwhile; an output's 16 values are the same either way.
// Writing and finishing are instantiated once per domain half, like the K loop: with a run-time `h` the accumulator registers
// are picked by a wave-uniform but DYNAMIC index, which hipcc lowers to s_set_gpr_idx moves through a 16-register VGPR copy of
// each tile -- that copy was the kernel's 16 - 50 spilled VGPRs.  Only the register selection is
// specialised; every barrier is ONE instruction that every wave of the workgroup reaches on the same path (the two
// halves used to meet at two different s_barrier instructions, which works on gfx950's arrival-counting barrier but is not
// defined behaviour).  The barriers wait for the LDS only: the stores behind them, and with NPART = 2 the next item's patch
// DMA, stay in flight.
// ---------------- epilogue: Y = A^T m A (A^T = [1 1 1 0; 0 1 -1 -1]), (factor,) shift, activation, residual, NCHW store.
// D = U^T-rows x tile-columns: the lane is tile `lane & 31` of the pair and register r is cout 8 (r >> 2) + 4 (lane >> 5) + (r & 3).
// Memory traffic of the epilogue is straight-line code, so that every wait hipcc places is an exact vmcnt(N) and no iteration
// waits for the round trip of its own loads (they used to: 8 per wave, 16 with a residual, all waves of the CU in lockstep):
//   * the 8 shifts (and factors) of the wave's registers are loaded once, in front of the exchange (`mid`, the persistent
//     kernel's hand-over to the next item, runs behind them);
//   * the residual and the output go through buffer descriptors, one per cout register: the descriptor's base carries
//     (b, cout) -- scalar arithmetic --, the lane keeps two 32-bit row offsets for all 8 registers, and the hardware bounds
//     check drops what must not be touched: offset 0xFFFFFFF0 for pixels outside the image, the descriptor's end for couts
//     past Cout, a descriptor of zero records where there is no residual (it reads as 0.0f: the `+ 0.f` of before);
//   * the residual of register r + 1 is requested before register r is finished.
constexpr uint32_t kWinoOutside = 0xFFFFFFF0u;
// One accumulator element -> VGPR.  Written out because hipcc, given plain element reads in an epilogue that keeps more than a
// few values live, turns the accumulator tiles into VGPR tuples behind the K loop: 128 v_accvgpr_read in one block and
// 20 - 60 spilled registers.  An asm statement is not padded for the MFMA -> read hazard: wino_acc_settle() goes first.
__device__ __forceinline__ float wino_acc_read(float a) {
    float t;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(t) : "a"(a));
    return t;
}
// The hazard (CDNA3 / CDNA4 ISA guide, "Manually inserted wait states", rows "XDL write VGPR -> VALU read / write of that
// VGPR", which cover v_accvgpr_read of an MFMA's D): 5 / 7 / 11 / 19 wait states behind an MFMA of 2 / 4 / 8 / 16 passes.
// v_mfma_f32_32x32x2_f32 (K10) is 16 passes, v_mfma_f32_32x32x16_f16 (K10h) 8 on gfx950 (16 at most): 19 states cover both,
// two `s_nop 15` are 32.  hipcc pads the hazard only for its own instructions, not for what an asm statement holds, so:
// the operands (one element of each of the 8 tiles: an MFMA writes its whole tile) tie the statement behind the last MFMA of
// every tile, and volatile statements keep their order, so every wino_acc_read comes after it.  Check after a compiler
// change: the two s_nop 15 stand between the last v_mfma and the first v_accvgpr_read in the disassembly of all kernels
// (tools/kernel_resources.sh does not see this).
__device__ __forceinline__ void wino_acc_settle(const f32x16 (&acc)[8]) {
    asm volatile("s_nop 15\n\ts_nop 15" ::"a"(acc[0][0]), "a"(acc[1][0]), "a"(acc[2][0]), "a"(acc[3][0]), "a"(acc[4][0]),
                 "a"(acc[5][0]), "a"(acc[6][0]), "a"(acc[7][0]));
}
// s_waitcnt lgkmcnt(0) + s_barrier: a barrier for LDS traffic that leaves global stores and LDS-DMA in flight
// (__syncthreads() drains them: vmcnt(0))
__device__ __forceinline__ void wino_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int TWV, bool FAC, int NPART, bool WE, class P, class Mid>
__device__ __forceinline__ void wino_exchange_store(const P& p, const float* fac, f32x16 (&acc)[8], float* xchg, int h, int pr,
                                                    int lane, int nb, int b, int ty0, int tx0, Mid mid) {
    static_assert(NPART == 1 || NPART == 2, "one exchange of 8 cout registers or two of 4");
    wino_acc_settle(acc);
    constexpr int RW = 32 / TWV, RP = 8 / NPART;           // RP: cout registers per exchange
    const int li = lane & 31, kk = lane >> 5;
    const int lr = pr * RW + li / TWV, lc = li % TWV;
    const bool h0 = h == 0;                                // wave-uniform
    const int oy0 = 2 * (ty0 + lr), ox = 2 * (tx0 + lc);
    const size_t hw = (size_t)p.H * p.W;
    const int cb = nb * 32 + 16 * h;                       // cout of register r8 = 0 in lane half 0 (uniform)
    auto cout_of = [](int r8) { return 8 * (r8 >> 2) + (r8 & 3); };
    // byte offsets of the lane's two output rows (and of their second pixel where it is accessed on its own) relative to
    // plane (b, cb + cout_of(r8)): < 20 H W, which the entry points keep below 2^32
    uint32_t vo[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const bool ok = ox < p.W && oy0 + a < p.H;
        const uint32_t o = (uint32_t)(((size_t)(4 * kk) * hw + (size_t)(oy0 + a) * p.W + ox) * 4);
        vo[a][0] = ok ? o : kWinoOutside;
        vo[a][1] = ok && ox + 1 < p.W ? o + 4 : kWinoOutside;
    }
    const size_t plane0 = ((size_t)b * p.Cout + cb) * hw;
    // descriptor over the planes of register r8 that exist: lane half 1 (4 couts further) falls off its end when they do not
    auto desc = [&](const float* base, int r8) {
        const int rem = p.Cout - cb - cout_of(r8);
        const uint32_t n = base == nullptr || rem <= 0 ? 0u : (uint32_t)((size_t)(rem < 5 ? rem : 5) * hw * 4);
        return __builtin_amdgcn_make_buffer_rsrc((void*)((base == nullptr ? p.y : base) + plane0 + (size_t)cout_of(r8) * hw), 0, n,
                                                 0x00020000);
    };
    // shifts and factors of the lane's 8 couts (a cout past Cout, or no shift at all, reads as 0.0f and is never stored)
    float sh[8], fc[8], rn[4];
    {
        const auto ss = __builtin_amdgcn_make_buffer_rsrc((void*)(p.shift != nullptr ? p.shift : p.y), 0,
                                                          p.shift != nullptr ? (uint32_t)p.Cout * 4u : 0u, 0x00020000);
        const auto fs = __builtin_amdgcn_make_buffer_rsrc((void*)(FAC ? fac : p.y), 0, FAC ? (uint32_t)p.Cout * 4u : 0u, 0x00020000);
        const uint32_t co4 = (uint32_t)(cb + 4 * kk) * 4;
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) {
            sh[r8] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ss, co4 + cout_of(r8) * 4, 0, 0));
            fc[r8] = FAC ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(fs, co4 + cout_of(r8) * 4, 0, 0)) : 1.f;
        }
    }
    // WE: W is even, so a lane's two pixels are one 8-byte access (ox is even); otherwise they go one by one
    auto res_issue = [&](int r8) {
        const auto rs = desc(p.res, r8);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (WE) {
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, vo[a][0], 0, 0);
                const uint32_t v0 = v[0], v1 = v[1];       // (a bit_cast of `v.y` itself reads element 0)
                rn[2 * a] = __builtin_bit_cast(float, v0);
                rn[2 * a + 1] = __builtin_bit_cast(float, v1);
            } else {
                rn[2 * a] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo[a][0], 0, 0));
                rn[2 * a + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo[a][1], 0, 0));
            }
        }
    };
    res_issue(0);
    __builtin_amdgcn_sched_barrier(0);
    mid();
    __builtin_amdgcn_sched_barrier(0);

    auto xwrite = [&](auto hc, int part) {
        constexpr int H = decltype(hc)::value;
        constexpr bool h0 = H == 0;
        float* mine = xchg + ((pr * 2 + H) * 8 * RP) * 64 + lane;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int q = 0; q < RP; ++q) mine[(k * RP + q) * 64] = wino_acc_read(h0 ? acc[k][8 + part * RP + q] : acc[k][part * RP + q]);
            __builtin_amdgcn_sched_barrier(0);             // (one accumulator tile at a time: few registers in flight)
        }
    };
    auto finish = [&](auto hc, int part) {
        constexpr int H = decltype(hc)::value;
        constexpr bool h0 = H == 0;
        const float* theirs = xchg + ((pr * 2 + (1 - H)) * 8 * RP) * 64 + lane;
        // One cout register per iteration, fenced by scheduling barriers: left alone, hipcc hoists the 64 exchange reads of
        // all eight unrolled iterations above the first store and spills 16 - 50 VGPRs beside the 128 live accumulators.
#pragma unroll
        for (int q = 0; q < RP; ++q) {
            __builtin_amdgcn_sched_barrier(0);
            const int r8 = part * RP + q;
            const float rc[4] = {rn[0], rn[1], rn[2], rn[3]};
            if (r8 + 1 < 8) res_issue(r8 + 1);            // one register ahead
            float m[4][4];                                 // m[i][j], xi = 4 i + j; rows 2h, 2h + 1 are this wave's
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float own = wino_acc_read(h0 ? acc[k][r8] : acc[k][8 + r8]);
                const float oth = theirs[(k * RP + q) * 64];
                m[k >> 2][k & 3] = h0 ? own : oth;
                m[2 + (k >> 2)][k & 3] = h0 ? oth : own;
            }
            float s[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[0][j] = m[0][j] + m[1][j] + m[2][j];
                s[1][j] = m[1][j] - m[2][j] - m[3][j];
            }
            const auto ws = desc(p.y, r8);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float y0 = FAC ? __builtin_fmaf(s[a][0] + s[a][1] + s[a][2], fc[r8], sh[r8]) : s[a][0] + s[a][1] + s[a][2] + sh[r8];
                float y1 = FAC ? __builtin_fmaf(s[a][1] - s[a][2] - s[a][3], fc[r8], sh[r8]) : s[a][1] - s[a][2] - s[a][3] + sh[r8];
                const float r0 = rc[2 * a], r1 = rc[2 * a + 1];
                if (p.res_first) { y0 += r0; y1 += r1; }
                y0 = act2d_exact(y0, p.act, p.slope);
                y1 = act2d_exact(y1, p.act, p.slope);
                if (!p.res_first) { y0 += r0; y1 += r1; }
                if (WE) {
                    __builtin_amdgcn_raw_buffer_store_b64((u32x2){__builtin_bit_cast(uint32_t, y0), __builtin_bit_cast(uint32_t, y1)},
                                                          ws, vo[a][0], 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, y0), ws, vo[a][0], 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, y1), ws, vo[a][1], 0, 0);
                }
            }
        }
    };
#pragma unroll
    for (int part = 0; part < NPART; ++part) {
        if (part > 0) wino_lds_barrier();                  // the partner has read the previous part
        if (h0) xwrite(std::integral_constant<int, 0>{}, part);
        else xwrite(std::integral_constant<int, 1>{}, part);
        wino_lds_barrier();
        if (h0) finish(std::integral_constant<int, 0>{}, part);
        else finish(std::integral_constant<int, 1>{}, part);
    }
}

// TWV: tiles per wave pair along x.  16 -> a pair is 2 x 16 tiles (4 x 32 pixels), a workgroup 8 x 16 tiles;
//                                    32 -> a pair is 1 x 32 tiles (2 x 64 pixels), a workgroup 4 x 32 tiles.
//
// 512 threads = 8 waves = 2 per SIMD.  Waves w and w + 4 form a PAIR on the same 32 tiles x 32 couts and split the
// Winograd domain: half h = w >> 2 owns the rows i in {2h, 2h + 1} of the 4 x 4 domain (xi = 4 i + j), i.e. 8
// accumulator tiles = 128 AGPRs.  A half needs only 3 of the 4 patch rows and 8 + 8 adds per patch.  After the loop the
// pair exchanges accumulators through LDS so that each wave finishes 8 of the 16 cout registers.
//
// What limits this kernel (measured on the 688 -> 320 level, 147 TF/s attainable at its tile padding): the fp32 MFMA
// runs at the fp32 VECTOR rate and every other instruction of the SIMD costs matrix-pipe time -- MFMAs + barriers
// alone 124 TF/s, + LDS reads -15, + transform adds -11, + DMA issue -10, in ANY arrangement tried: all 16 xi in one
// wave per SIMD (50 %: nothing hides its LDS waits), two waves in strict MFMA / prepare ping-pong phases (75 TF/s: the
// preparing wave does not run in the shadow of the partner's MFMAs), or the interleaved form below (93 TF/s).  So the
// loop is built to (a) issue every LDS read one block (8 MFMAs) before its use, (b) keep the instruction count per
// MFMA minimal (one instantiation per domain half: no selects; operands re-read per block: no register copies) and
// (c) let the two waves of a SIMD do their VALU work at different points of a block:
//     half 0:  reads(q+1) | 8 MFMAs(q)                      | transform(q+1)
//     half 1:  reads(q+1) | 4 MFMAs(q) | transform(q+1) | 4 MFMAs(q)
// sched_barrier(0) pins the segment order (hipcc otherwise sinks the reads to their first use); the last chunk is
// peeled so the loop body is straight-line code (exact s_waitcnt counts instead of lgkmcnt(0) at a control-flow join).
//
// Staging is LDS-DMA only (no staging VGPRs, no ds_write, no global_load results for hipcc to wait on):
//   patch : buffer_load_dword ... lds through a descriptor of image b's remaining channels -- the LDS image is
//           lane-linear ([cin][row][RS] floats, 64 consecutive floats per wave instruction), every lane supplies the
//           byte offset of ITS element, and the hardware bounds check provides both kinds of zero fill: lanes outside
//           the image (the convolution's padding, the row pad) carry an offset past the descriptor, channels past Cin
//           fall off its end;
//   U     : global_load_lds_dwordx4, one 1-KB fragment record per wave instruction, already in A-fragment order.
// Block (c, 3) reads chunk c+1, so the barrier (vmcnt(0): chunk c+1, issued a chunk earlier, has landed; every wave has
// issued its last reads of chunk c) sits in front of it and the DMA of chunk c+2 into chunk c's buffers follows it.
// EXP (development A/B switches, wrong results): 1 = no DMA after chunk 1, 2 = DMA only (no MFMA)
template <int TWV, bool WE, int EXP = 0>
__global__ void __launch_bounds__(512, 2) wino3x3_kernel(const WinoP p) {
    constexpr int RW = 32 / TWV;                 // tile rows per wave pair
    constexpr int WGR = 4 * RW;                  // tile rows per workgroup
    constexpr int PR = 2 * WGR + 2;              // patch rows / cols (one halo pixel each side)
    constexpr int PC = 2 * TWV + 2;
    // ds_read_b64 serves 32 lanes per cycle over 64 banks: a pair's two tile rows (TWV = 16) must sit 32 banks apart
    constexpr int RS = TWV == 16 ? 48 : 68;      // LDS row stride in floats
    constexpr int PLANE = PR * RS;
    constexpr int NEL = 8 * PLANE;               // floats of one staged chunk image (pads included)
    constexpr int NDMA = (NEL + 511) / 512;      // patch DMA instructions per wave per chunk
    constexpr int PBUF = NDMA * 512;             // floats per patch buffer (whole wave instructions)
    constexpr int UBUF = 16 * 256;               // floats per U buffer: 16 xi records of 64 lanes x 4
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [2][PBUF] patches, then [2][UBUF] weights

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pr = wave & 3, h = wave >> 2;      // tile group of the pair, half of the Winograd domain
    const int li = lane & 31, kk = lane >> 5;

    // XCD-aware bijective remap (cout blocks of one tile block stay on one XCD's L2: they re-read the same patch)
    const uint32_t bid = xcd_remap(blockIdx.x, p.nwg);
    const int nb = bid % p.nblk;
    uint32_t t = bid / p.nblk;
    const int bx = t % p.wg_tx;
    t /= p.wg_tx;
    const int by = t % p.wg_ty;
    const int b = t / p.wg_ty;
    const int ty0 = by * WGR, tx0 = bx * TWV;
    const int gy0 = 2 * ty0 - 1, gx0 = 2 * tx0 - 1;

    // chunk-invariant byte offset of this lane's element in each of its wave's DMA instructions (relative to the
    // chunk's first channel); 0xFFFFFFF0 = "outside": past any descriptor, the DMA writes 0.0f
    const size_t plane_hw = (size_t)p.H * p.W;
    uint32_t voff[NDMA];
#pragma unroll
    for (int i = 0; i < NDMA; ++i) {
        const int e = (wave * NDMA + i) * 64 + lane;
        const int cin = e / PLANE, rem = e - cin * PLANE;
        const int row = rem / RS, col = rem - row * RS;
        const int gy = gy0 + row, gx = gx0 + col;
        const bool ok = e < NEL && col < PC && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
        voff[i] = ok ? (uint32_t)((cin * plane_hw + (size_t)gy * p.W + gx) * 4) : 0xFFFFFFF0u;
    }
    const float* const xb = p.x + (size_t)b * p.Cin * plane_hw;
    const float* const ubase = p.upk + (size_t)nb * 256 + lane * 4;
    const size_t u_xi = (size_t)p.nblk * 256;            // floats per (chunk, xi) record

    auto issue_chunk = [&](int c) {
        const int buf = c & 1;
        // descriptor over channels [8c, Cin) of image b: offsets past the last channel read as zero
        const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (size_t)c * 8 * plane_hw), 0,
                                                            (uint32_t)((size_t)(p.Cin - c * 8) * plane_hw * 4), 0x00020000);
        float* pdst = lds + buf * PBUF + wave * NDMA * 64;
#pragma unroll
        for (int i = 0; i < NDMA; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, pdst + i * 64, 4, voff[i], 0, 0, 0);
        float* udst = lds + 2 * PBUF + buf * UBUF + wave * 2 * 256;
        const float* usrc = ubase + ((size_t)c * 16 + wave * 2) * u_xi;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds(usrc + (size_t)j * u_xi, udst + j * 256, 16, 0, 0);
    };

    // this lane's tile inside the workgroup and its patch corner in LDS (rows h .. h + 2 of the 4 x 4 patch)
    const int lr = pr * RW + li / TWV, lc = li % TWV;
    const int pbase = kk * 4 * PLANE + (2 * lr + h) * RS + 2 * lc;

    // An (empty) asm with an AGPR operand makes hipcc select the AGPR form of the MFMAs (at 2 waves per SIMD it would
    // otherwise put the accumulators in VGPRs, which leaves too few for the register-level prefetch below).
    asm volatile("" ::"a"(0.f));
    f32x16 acc[8];                                        // xi = 8 h + k
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    auto read_d = [&](const float* pl, int q, float (&d)[3][4]) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const f32x2 lo = *(const f32x2*)(pl + q * PLANE + r * RS);
            const f32x2 hi = *(const f32x2*)(pl + q * PLANE + r * RS + 2);
            d[r][0] = lo.x; d[r][1] = lo.y; d[r][2] = hi.x; d[r][3] = hi.y;
        }
    };
    // U records of a chunk: r = 4 q + 2 h + part, each [lane][4 xi] (see wino_pack_kernel): 2 x ds_read_b128 per cin
    auto read_u = [&](int buf, int q, float (&u)[8]) {
        const f32x4* ul = (const f32x4*)(lds + 2 * PBUF + buf * UBUF) + ((q * 4 + h * 2) * 64 + lane);
        const f32x4 a = ul[0], b4 = ul[64];
        u[0] = a.x; u[1] = a.y; u[2] = a.z; u[3] = a.w; u[4] = b4.x; u[5] = b4.y; u[6] = b4.z; u[7] = b4.w;
    };
    const bool h0 = h == 0;                                // wave-uniform
    auto transform = [&](auto hc, const float (&d)[3][4], float (&v)[8]) {
        constexpr bool h0 = decltype(hc)::value == 0;
        // rows 2h, 2h + 1 of B^T d (B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]); d holds patch rows h, h+1, h+2:
        //   h = 0: d0 - d2, d1 + d2        h = 1 (d = rows 1, 2, 3): d2 - d1, d1 - d3
        float tt[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tt[0][j] = h0 ? d[0][j] - d[2][j] : d[1][j] - d[0][j];
            tt[1][j] = h0 ? d[1][j] + d[2][j] : d[0][j] - d[2][j];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {                      // (B^T d) B
            v[4 * i + 0] = tt[i][0] - tt[i][2];
            v[4 * i + 1] = tt[i][1] + tt[i][2];
            v[4 * i + 2] = tt[i][2] - tt[i][1];
            v[4 * i + 3] = tt[i][1] - tt[i][3];
        }
    };
    auto mfma4 = [&](const float (&u)[8], const float (&v)[8], int k0) {
#pragma unroll
        for (int k = k0; k < k0 + 4; ++k) {
            if (EXP == 2) acc[k][0] += u[k] * v[k];
            else acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(u[k], v[k], acc[k], 0, 0, 0);
        }
    };

    issue_chunk(0);
    __syncthreads();                                      // (drains the DMA: vmcnt(0) + barrier)
    if (p.chunks > 1) issue_chunk(1);

    // The whole K loop is instantiated once per domain half (a wave-uniform branch): no per-lane selects inside.
    auto k_loop = [&](auto hc) {
        constexpr bool first_half = decltype(hc)::value == 0;
        float d[3][4], ua[8], ub[8], va[8], vb[8];         // (a, b): register sets alternating per block, no copies
        // one block: operands (u_cur, v_cur) of cin q; prefetch + transform of the next block into (u_nxt, v_nxt)
        auto block = [&](const float* pl_nxt, int buf_nxt, int q_nxt, float (&u_cur)[8], float (&v_cur)[8],
                         float (&u_nxt)[8], float (&v_nxt)[8]) {
            read_d(pl_nxt, q_nxt, d);
            read_u(buf_nxt, q_nxt, u_nxt);
            __builtin_amdgcn_sched_barrier(0);
            mfma4(u_cur, v_cur, 0);
            if (first_half) {
                mfma4(u_cur, v_cur, 4);
                __builtin_amdgcn_sched_barrier(0);
                transform(hc, d, v_nxt);
            } else {
                __builtin_amdgcn_sched_barrier(0);
                transform(hc, d, v_nxt);
                __builtin_amdgcn_sched_barrier(0);
                mfma4(u_cur, v_cur, 4);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        read_d(lds + pbase, 0, d);
        read_u(0, 0, ua);
        transform(hc, d, va);
        for (int c = 0; c + 1 < p.chunks; ++c) {
            const float* pl = lds + (c & 1) * PBUF + pbase;
            const float* pn = lds + ((c + 1) & 1) * PBUF + pbase;
            block(pl, c & 1, 1, ua, va, ub, vb);
            block(pl, c & 1, 2, ub, vb, ua, va);
            block(pl, c & 1, 3, ua, va, ub, vb);
            __syncthreads();                               // vmcnt(0) + lgkmcnt(0) + barrier
            if (EXP != 1 && c + 2 < p.chunks) issue_chunk(c + 2);
            block(pn, (c + 1) & 1, 0, ub, vb, ua, va);
        }
        const int lb = (p.chunks - 1) & 1;
        const float* pl = lds + lb * PBUF + pbase;
        block(pl, lb, 1, ua, va, ub, vb);
        block(pl, lb, 2, ub, vb, ua, va);
        block(pl, lb, 3, ua, va, ub, vb);
        mfma4(ub, vb, 0);
        mfma4(ub, vb, 4);
    };
    if (h0) k_loop(std::integral_constant<int, 0>{});
    else k_loop(std::integral_constant<int, 1>{});
    __syncthreads();                                       // every wave is done with the staging buffers

    wino_exchange_store<TWV, false, 1, WE>(p, nullptr, acc, lds, h, pr, lane, nb, b, ty0, tx0, [] {});
}

// upk[chunk][r = 4 q + 2 h + part][cout/32][lane][j]: the A operands of cin 8 chunk + 4 (lane >> 5) + q for the four
// Winograd positions xi = 8 h + 4 part + j of cout = blk*32 + (lane & 31); value (G g G^T)[xi] * scale[cout], zero
// outside (cout, cin).  One record = what a wave half h needs for one cin step, as two lane-linear 1-KB pieces.
// G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]; float64 arithmetic.
__global__ void wino_pack_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ upk,
                                 int cout, int cin, int nblk, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = i & 3, lane = (i >> 2) & 63;
    long t = i >> 8;
    const int blk = t % nblk; t /= nblk;
    const int rec = t & 15;
    const int chunk = (int)(t >> 4);
    const int q = rec >> 2, hh = (rec >> 1) & 1, part = rec & 1;
    const int xi = 8 * hh + 4 * part + j;
    const int co = blk * 32 + (lane & 31), ci = chunk * 8 + (lane >> 5) * 4 + q;
    float out = 0.f;
    if (co < cout && ci < cin) {
        const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        const float* g = w + ((size_t)co * cin + ci) * 9;
        const int a = xi >> 2, bcol = xi & 3;
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int n = 0; n < 3; ++n) s += G[a][m] * (double)g[m * 3 + n] * G[bcol][n];
        if (scale != nullptr) s *= (double)scale[co];
        out = (float)s;
    }
    upk[i] = out;
}

// K10h -- K10 on the f16 matrix pipe with the two-term fp16 split (the scheme of K2s3h, csrc/conv3d_c32p.hip): same contract,
// same tiling (8 waves, a pair of waves owns 32 tiles x 32 couts and 8 Winograd positions each), same exchange and epilogue.
//   U' = 2^k[co] (G g G^T scale[co]) = hi_u + lo_u          (packed: occd_wino_pack_weights_f16x2, max|U'| in [2^13, 2^14))
//   V' = 2^kWinoStageExp (B^T d B)   = hi_v + 2^-11 lo'_v   (split in the kernel, after the float32 transform)
//   acc += lo_u hi_v + (2^-11 hi_u) lo'_v + hi_u hi_v       three v_mfma_f32_32x32x16_f16 per position and 16 cins, smallest
//                                                           terms first; 2^-11 hi_u is one v_pk_mul_f16 per two elements
//   y = act(fac[co] (A^T acc A) + shift) (+ res),           fac = 2^-(k + kWinoStageExp)
// |V| <= 4 max|x| and fp16 rounds to Inf from 65520 on, so finite activations with |x| >= 65520 / (4 * 2^kWinoStageExp) = 8190
// can overflow hi_v and give non-finite outputs in the pixels their patches reach.
// What differs from K10's loop:
//   * a chunk is 16 cins, staged as two 8-cin images (K10's DMA pattern twice); lane half kk owns cins 8 kk .. 8 kk + 7 --
//     the 8 k values of its B fragment -- and transforms their 4x4 patches two cins at a time (a pair of cins is one packed
//     fp16 register per position and term);
//   * the loop is bound by vector issue, not by the matrix pipe (24 MFMAs = 768 pipe cycles per wave and chunk against some
//     500 VALU / LDS instructions), so it is plain program order, one ROW of the wave's half of the domain at a time (4
//     positions: 32 operand VGPRs): transform + split row 0 | barrier | 12 MFMAs | transform + split row 1 | 12 MFMAs |
//     barrier.  A row needs two patch rows, so a chunk costs 64 ds_read_b64 where all 8 positions at once would cost 48 --
//     and 64 operand VGPRs, which spill next to the DMA offsets;
//   * U (two fp16 images in A-fragment order, 32 KB per chunk and cout block, LDS-DMA as in K10) is single-buffered (a second
//     buffer does not fit beside the patches of the 2 x 16 tiling): the first barrier is where it (and the next patch) has
//     landed, under the transform of row 0; the second frees it.
//     Both barriers sit in the one loop body that every wave runs; only the transform is instantiated per domain half.
constexpr int kWinoStageExp = 1;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

struct WinoHP {
    const float* x;
    const uint16_t* upk;
    const float* fac;
    const float* shift;
    const float* res;
    float* y;
    int B, Cin, Cout, H, W;
    int chunks, nblk, wg_ty, wg_tx, nwg;
    int act, res_first;
    float slope;
};

// (a, b) = the values of one Winograd position for two consecutive cins -> packed hi and lo' terms.  The residuals are
// fma(hi, -2^11, 2^11 x) on the fp16 hi (one mixed-precision fma each, no conversion back; both products are exact, so
// this is (x - hi) 2^11 to the bit).  The empty asm keeps the SLP vectoriser from packing the transform and the residuals
// into v_pk_*_f32: packed float32 VALU instructions beside MFMAs cost more than the two scalar ones they replace.
__device__ __forceinline__ void split2_f16x2(float a, float b, uint32_t& hi, uint32_t& lo) {
    asm("" : "+v"(a));
    asm("" : "+v"(b));
    const f16x2 h = __builtin_convertvector((f32x2){a, b}, f16x2);
    float r0 = __builtin_fmaf((float)h[0], -2048.f, a * 2048.f);
    float r1 = __builtin_fmaf((float)h[1], -2048.f, b * 2048.f);
    asm("" : "+v"(r0));
    asm("" : "+v"(r1));
    hi = __builtin_bit_cast(uint32_t, h);
    lo = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){r0, r1}, f16x2));
}

// One ROW of the Winograd domain for the lane's 8 cins, shared by wino3x3_f16x2_kernel (row i of the wave's half h: xi = 8 h +
// 4 i + j) and wino3x3_f16x2_pair_kernel (row 2 h + i).  Row 2h + i of B^T d needs two patch rows (B^T = [1 0 -1 0; 0 1 1 0;
// 0 -1 1 0; 0 1 0 -1]; rows counted from patch row h, where `pl` points):
//   h = 0: i = 0: d0 - d2, i = 1: d1 + d2        h = 1: i = 0: d1 - d0, i = 1: d0 - d2
// then (.) B with the staging factor 2^kWinoStageExp riding on it: 2 t_a -+ 2 t_b is one fma of t_a against the doubled
// t_b, exactly 2 (t_a -+ t_b).  Two cins at a time: a pair is one packed fp16 register per position and term.
// PLANE, RS: floats of one staged cin plane and of one of its rows.  vh, vl: [position of the row][cin pair].
static_assert(kWinoStageExp == 1, "the transform below stages 2 V");
template <int H, int I, int PLANE, int RS>
__device__ __forceinline__ void wino_row_v(const float* pl, uint32_t (&vh)[4][4], uint32_t (&vl)[4][4]) {
    constexpr int RA = H == 0 ? I : 1 - I, RB = H == 1 && I == 0 ? 0 : 2;
    constexpr bool ADD = H == 0 && I == 1;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float v[2][4];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float* pq = pl + (2 * m + e) * PLANE;
            const f32x2 a0 = *(const f32x2*)(pq + RA * RS), a1 = *(const f32x2*)(pq + RA * RS + 2);
            const f32x2 b0 = *(const f32x2*)(pq + RB * RS), b1 = *(const f32x2*)(pq + RB * RS + 2);
            float ra[4] = {a0.x, a0.y, a1.x, a1.y};
#pragma unroll
            for (int j = 0; j < 4; ++j) asm("" : "+v"(ra[j]));          // (scalar adds: see split2_f16x2)
            const float t0 = ADD ? ra[0] + b0.x : ra[0] - b0.x, t1 = ADD ? ra[1] + b0.y : ra[1] - b0.y;
            const float t2 = ADD ? ra[2] + b1.x : ra[2] - b1.x, t3 = ADD ? ra[3] + b1.y : ra[3] - b1.y;
            const float u1 = 2.f * t1, u2 = 2.f * t2;
            v[e][0] = __builtin_fmaf(2.f, t0, -u2);
            v[e][1] = u1 + u2;
            v[e][2] = u2 - u1;
            v[e][3] = __builtin_fmaf(-2.f, t3, u1);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) split2_f16x2(v[0][j], v[1][j], vh[j][m], vl[j][m]);
    }
}

// PERSIST: a workgroup walks the items v = blockIdx.x, blockIdx.x + gridDim.x, ... < nwg (a static assignment: no queue, no
// flags, nothing shared between workgroups, any grid size is correct) and hands over inside the epilogue:
//     last barrier of the K loop | shifts, factors, first residual requested | next item: DMA offsets, descriptor, patch DMA
//     of its chunk 0 into patch buffer 0 | exchange registers 0-3: write, barrier, finish, store | barrier | registers 4-7:
//     write, barrier, finish, store | next item's first barrier (vmcnt(0): its patch 0 has landed, and every wave has read
//     the second exchange) | issue_u(0), issue_patch(1), ...
// The two-part exchange (64 KB) lives behind patch buffer 0, over patch buffer 1 and U, which are dead until that barrier.
// With a grid that is a multiple of 8, v % 8 is the same for all items of a workgroup, so xcd_remap still puts the cout blocks
// of one tile block on one XCD, one round at a time.  !PERSIST: one item per workgroup, one 128-KB exchange over everything.
template <int TWV, bool PERSIST, bool WE>
__global__ void __launch_bounds__(512, 2) wino3x3_f16x2_kernel(const WinoHP p) {
    constexpr int RW = 32 / TWV;                 // (tile geometry and LDS row stride: see wino3x3_kernel)
    constexpr int WGR = 4 * RW;
    constexpr int PR = 2 * WGR + 2;
    constexpr int PC = 2 * TWV + 2;
    constexpr int RS = TWV == 16 ? 48 : 68;
    constexpr int PLANE = PR * RS;
    constexpr int NEL = 8 * PLANE;               // floats of one staged 8-cin image
    constexpr int NDMA = (NEL + 511) / 512;
    constexpr int PBUF = NDMA * 512;
    constexpr int UOFF = 4 * PBUF;               // [2 buffers][2 x 8 cins][PBUF] patches, then 32 records of U (32 KB)
    constexpr int XOFF = PERSIST ? 2 * PBUF : 0; // the exchange: behind patch buffer 0, or over everything
    constexpr int XFLOATS = 4 * 2 * 64 * 64 / (PERSIST ? 2 : 1);
    static_assert(XOFF + XFLOATS <= (PERSIST ? UOFF + 32 * 256 : 4 * 2 * 64 * 64), "the exchange must fit in the staging buffers");
    static_assert((UOFF + 32 * 256) * 4 <= 160 * 1024 && (XOFF + XFLOATS) * 4 <= 160 * 1024, "LDS of a CU");
    static_assert(XOFF % 4 == 0, "16-byte aligned exchange");
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const size_t plane_hw = (size_t)p.H * p.W;
    const size_t u_rec = (size_t)p.nblk * 512;           // halves per (chunk, xi, image) record
    uint32_t voff[NDMA];                          // as in wino3x3_kernel: 0xFFFFFFF0 = outside, the DMA writes 0.0f
    int nb, b, ty0, tx0;                          // the item: cout block, image, first tile
    // (the lane index is taken from a thread id the compiler cannot match with earlier ones: kept live across the K loop,
    // the lane's indices are the registers it spills)
    auto fresh_tid = [] {
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return t;
    };
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int pr = wave & 3, h = wave >> 2;
    const bool h0 = h == 0;                                // wave-uniform

    auto setup = [&](uint32_t v) {                        // item v: where it is, and this lane's DMA offsets in it
        const uint32_t bid = xcd_remap(v, p.nwg);
        nb = bid % p.nblk;
        uint32_t t = bid / p.nblk;
        const int bx = t % p.wg_tx;
        t /= p.wg_tx;
        const int by = t % p.wg_ty;
        b = t / p.wg_ty;
        ty0 = by * WGR, tx0 = bx * TWV;
        const int gy0 = 2 * ty0 - 1, gx0 = 2 * tx0 - 1;
        const int lane = fresh_tid() & 63;
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int e = (wave * NDMA + i) * 64 + lane;
            const int cin = e / PLANE, rem = e - cin * PLANE;
            const int row = rem / RS, col = rem - row * RS;
            const int gy = gy0 + row, gx = gx0 + col;
            const bool ok = e < NEL && col < PC && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            voff[i] = ok ? (uint32_t)((cin * plane_hw + (size_t)gy * p.W + gx) * 4) : 0xFFFFFFF0u;
        }
    };
    auto issue_patch = [&](int c, bool live = true) {
        const float* const xb = p.x + (size_t)b * p.Cin * plane_hw;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // descriptor over channels [16 c + 8 s, Cin) of image b; none left (or !live): zero records, every lane reads 0.0f
            const int ch0 = c * 16 + s * 8, left = live ? p.Cin - ch0 : 0;
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (size_t)(left > 0 ? ch0 : 0) * plane_hw), 0,
                                                                left > 0 ? (uint32_t)((size_t)left * plane_hw * 4) : 0u, 0x00020000);
            float* pdst = lds + ((c & 1) * 2 + s) * PBUF + wave * NDMA * 64;
#pragma unroll
            for (int i = 0; i < NDMA; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, pdst + i * 64, 4, voff[i], 0, 0, 0);
        }
    };

    asm volatile("" ::"a"(0.f));                          // AGPR accumulators (see wino3x3_kernel)
    f32x16 acc[8];                                        // xi = 8 h + k

    // the 12 MFMAs of row i against the U records r = 2 xi + image of this chunk; positions in two interleaved pairs so
    // that no MFMA waits on its predecessor
    auto row_m = [&](auto ic, const u32x4* ul, const uint32_t (&vh)[4][4], const uint32_t (&vl)[4][4]) {
        constexpr int I = decltype(ic)::value;
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            f16x8 uh[2], ulo[2], us[2], bh[2], bl[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                uh[e] = __builtin_bit_cast(f16x8, ul[(2 * (4 * I + j + e)) * 64]);
                ulo[e] = __builtin_bit_cast(f16x8, ul[(2 * (4 * I + j + e) + 1) * 64]);
                us[e] = uh[e] * (_Float16)(1.f / 2048.f);
                bh[e] = __builtin_bit_cast(f16x8, (u32x4){vh[j + e][0], vh[j + e][1], vh[j + e][2], vh[j + e][3]});
                bl[e] = __builtin_bit_cast(f16x8, (u32x4){vl[j + e][0], vl[j + e][1], vl[j + e][2], vl[j + e][3]});
            }
#pragma unroll
            for (int e = 0; e < 2; ++e)
                acc[4 * I + j + e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ulo[e], bh[e], acc[4 * I + j + e], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 2; ++e)
                acc[4 * I + j + e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(us[e], bl[e], acc[4 * I + j + e], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 2; ++e)
                acc[4 * I + j + e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(uh[e], bh[e], acc[4 * I + j + e], 0, 0, 0);
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;

    uint32_t v = blockIdx.x;
    setup(v);
    issue_patch(0);
    for (;;) {
        const int lane = fresh_tid() & 63;
        const int li = lane & 31, kk = lane >> 5;
        const int lr = pr * RW + li / TWV, lc = li % TWV;
        const int pbase = kk * PBUF + (2 * lr + h) * RS + 2 * lc;
        const u32x4* const ul = (const u32x4*)(lds + UOFF) + (h * 16 * 64 + lane);
        const uint16_t* const ubase = p.upk + (size_t)nb * 512 + lane * 8;
        auto issue_u = [&](int c) {                       // 32 records of 1 KB: r = 2 xi + image (0 hi, 1 lo), 4 per wave
            float* udst = lds + UOFF + wave * 4 * 256;
            const uint16_t* usrc = ubase + ((size_t)c * 32 + wave * 4) * u_rec;
#pragma unroll
            for (int j = 0; j < 4; ++j) __builtin_amdgcn_global_load_lds(usrc + (size_t)j * u_rec, udst + j * 256, 16, 0, 0);
        };
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

        __syncthreads();                                   // (vmcnt(0) + barrier: patch 0 has landed; the exchange is read)
        for (int c = 0; c < p.chunks; ++c) {
            issue_u(c);
            if (c + 1 < p.chunks) issue_patch(c + 1);
            const float* pl = lds + (c & 1) * 2 * PBUF + pbase;
            uint32_t ah[4][4], al[4][4], bh[4][4], bl[4][4];   // [position of the row][cin pair]: B fragments, hi and lo' terms
            if (h0) wino_row_v<0, 0, PLANE, RS>(pl, ah, al);
            else wino_row_v<1, 0, PLANE, RS>(pl, ah, al);
            __syncthreads();                               // U of chunk c has landed (vmcnt(0): so has the patch of chunk c + 1)
            row_m(I0{}, ul, ah, al);                       // ... and run under the transform of the second row
            if (h0) wino_row_v<0, 1, PLANE, RS>(pl, bh, bl);
            else wino_row_v<1, 1, PLANE, RS>(pl, bh, bl);
            row_m(I1{}, ul, bh, bl);
            __syncthreads();                               // every wave is done with U and the patch of chunk c; patch c + 1 has landed
        }

        // ---------------- pair exchange and epilogue (shared with K10), with the per-cout factor; the next item's first patch
        // is requested from inside it
        const int nb_c = nb, b_c = b, ty0_c = ty0, tx0_c = tx0;
        const uint32_t vn = v + gridDim.x;
        const bool more = PERSIST && vn < (uint32_t)p.nwg;
        wino_exchange_store<TWV, true, PERSIST ? 2 : 1, WE>(p, p.fac, acc, lds + XOFF, h, pr, fresh_tid() & 63, nb_c, b_c, ty0_c, tx0_c, [&] {
            // No branch around the DMA: behind a uniform `if (more)` hipcc takes the smaller pending count at the join, and
            // the epilogue's first counted waits then drain the 2 x NDMA patch requests as well.  The last item of a
            // workgroup requests its own patch again through descriptors of zero records: nothing is read.
            if (PERSIST) {
                setup(more ? vn : v);
                issue_patch(0, more);
            }
        });
        if (!more) {
            // (the zero-record DMA still writes LDS: it must have landed before the workgroup gives its LDS back)
            if (PERSIST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            break;
        }
        v = vn;
    }
}

// K10h, cout-pair form: a work item is (cout blocks 2q and 2q + 1, image, block of 64 tiles), so that the patch DMA, the LDS
// reads, the transform and the split of a tile block are done once for two cout blocks, not once for each.
//   * a QUAD of waves (g = wave >> 2) owns 32 tiles x 64 couts; wave `row` = wave & 3 of it owns row `row` of the 4 x 4 domain
//     (xi = 4 row + j) for BOTH blocks: acc[4 blk + j], 128 AGPRs as before, 24 MFMAs per wave and chunk as before, but one
//     row transform per chunk where wino3x3_f16x2_kernel runs two.  A workgroup is 2 x 32 (TWV = 32) or 4 x 16 tiles;
//   * per accumulator the MFMAs come in the order of wino3x3_f16x2_kernel (lo_u hi_v, hs_u lo'_v, hi_u hi_v; chunks ascending)
//     and the epilogue adds in the order of wino_exchange_store's finish(), so every output has the bits of that kernel;
//   * U of one chunk is 64 records (64 KB, single-buffered as before): record 32 blk + 2 xi + image, 8 per wave.  With an odd
//     number of cout blocks the last pair has no second block (`live1`, uniform over the workgroup): its U is not requested,
//     its MFMAs and its half of the epilogue are skipped, nothing is read or written for it;
//   * one item per workgroup only (no persistent grid).
// Measured (profiles/wino_cout_pair_ab.txt): 0.17 ms per frame of a 0.32 - 0.50 ms bound.  The likeliest reason, NOT measured:
// a chunk's U (twice K10h's request) is asked for and waited for inside the chunk behind ONE row transform, half of K10h's
// window; staging block 1's records under block 0's MFMAs is the untried remedy.
// The transform is wino_row_v, shared with wino3x3_f16x2_kernel (the reference for bit equality); the MFMA block is that
// kernel's with the cout block added to the accumulator and U record indices.
// The quad exchange and the epilogue of the cout-pair form.  Wave `row` finishes the cout registers 4 row .. 4 row + 3 of both
// blocks (r8 = 4 blk + t: cout 32 (nb0 + blk) + 8 row + 4 (lane >> 5) + t) and needs the 12 positions of the three other waves
// of its quad for them: the RAW accumulators go through xchg[quad][reader][writer slot][j][t][lane], one block per exchange
// (96 KB each, over the staging buffers, which are dead behind the caller's last barrier).  The arithmetic, the descriptors
// and the order of the memory traffic are those of wino_exchange_store, REPEATED here, not shared: with the offsets, the
// descriptor, the residual load and the store tail taken from common helpers hipcc schedules the epilogues of K10 and K10h
// differently (every kernel of this file changed), and those two stay instruction for instruction what was measured.  A change
// to the float operations there must be made here too; tests/test_wino_cout_pair.py compares the two bit for bit.
// Writing and finishing are instantiated once per row,
// every barrier is one instruction that all waves of the workgroup reach on one path (`live1` is uniform over the workgroup).
template <int TWV, bool WE>
__device__ __forceinline__ void wino_quad_exchange_store(const WinoHP& p, f32x16 (&acc)[8], float* xchg, int row, int g, int lane,
                                                         int nb0, bool live1, int b, int ty0, int tx0) {
    wino_acc_settle(acc);
    constexpr int RW = 32 / TWV;
    const int li = lane & 31, kk = lane >> 5;
    const int lr = g * RW + li / TWV, lc = li % TWV;
    const int oy0 = 2 * (ty0 + lr), ox = 2 * (tx0 + lc);
    const size_t hw = (size_t)p.H * p.W;
    const int cb = nb0 * 32 + 8 * row;                     // cout of register r8 = 0 in lane half 0 (uniform)
    auto cout_of = [](int r8) { return 32 * (r8 >> 2) + (r8 & 3); };
    uint32_t vo[2][2];                                     // (as in wino_exchange_store)
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const bool ok = ox < p.W && oy0 + a < p.H;
        const uint32_t o = (uint32_t)(((size_t)(4 * kk) * hw + (size_t)(oy0 + a) * p.W + ox) * 4);
        vo[a][0] = ok ? o : kWinoOutside;
        vo[a][1] = ok && ox + 1 < p.W ? o + 4 : kWinoOutside;
    }
    const size_t plane0 = ((size_t)b * p.Cout + cb) * hw;
    // descriptor over the planes of register r8 that exist; none do for a second block that does not
    auto desc = [&](const float* base, int r8) {
        const int rem = p.Cout - cb - cout_of(r8);
        const uint32_t n = base == nullptr || rem <= 0 ? 0u : (uint32_t)((size_t)(rem < 5 ? rem : 5) * hw * 4);
        return __builtin_amdgcn_make_buffer_rsrc((void*)((base == nullptr ? p.y : base) + plane0 + (size_t)cout_of(r8) * hw), 0, n,
                                                 0x00020000);
    };
    float sh[8], fc[8], rn[4];
    {
        const auto ss = __builtin_amdgcn_make_buffer_rsrc((void*)(p.shift != nullptr ? p.shift : p.y), 0,
                                                          p.shift != nullptr ? (uint32_t)p.Cout * 4u : 0u, 0x00020000);
        const auto fs = __builtin_amdgcn_make_buffer_rsrc((void*)p.fac, 0, (uint32_t)p.Cout * 4u, 0x00020000);
        const uint32_t co4 = (uint32_t)(cb + 4 * kk) * 4;
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) {
            sh[r8] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ss, co4 + cout_of(r8) * 4, 0, 0));
            fc[r8] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(fs, co4 + cout_of(r8) * 4, 0, 0));
        }
    }
    auto res_issue = [&](int r8) {
        const auto rs = desc(p.res, r8);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            if (WE) {
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, vo[a][0], 0, 0);
                const uint32_t v0 = v[0], v1 = v[1];
                rn[2 * a] = __builtin_bit_cast(float, v0);
                rn[2 * a + 1] = __builtin_bit_cast(float, v1);
            } else {
                rn[2 * a] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo[a][0], 0, 0));
                rn[2 * a + 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, vo[a][1], 0, 0));
            }
        }
    };
    res_issue(0);
    __builtin_amdgcn_sched_barrier(0);

    // writer row I -> slot of the three a reader keeps for the other rows
    auto xwrite = [&](auto ic, int blk) {
        constexpr int I = decltype(ic)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int rd = 0; rd < 4; ++rd) {
                if (rd == I) continue;
                float* dst = xchg + (((g * 4 + rd) * 3 + (I < rd ? I : I - 1)) * 16 + j * 4) * 64 + lane;
#pragma unroll
                for (int t = 0; t < 4; ++t) dst[t * 64] = wino_acc_read(acc[blk * 4 + j][4 * rd + t]);
            }
            __builtin_amdgcn_sched_barrier(0);             // (one accumulator tile at a time: few registers in flight)
        }
    };
    auto finish = [&](auto ic, int blk) {
        constexpr int I = decltype(ic)::value;
        const float* theirs = xchg + ((g * 4 + I) * 3 * 16) * 64 + lane;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            __builtin_amdgcn_sched_barrier(0);             // (one cout register per iteration: see wino_exchange_store)
            const int r8 = blk * 4 + t;
            const float rc[4] = {rn[0], rn[1], rn[2], rn[3]};
            if (r8 + 1 < 8) res_issue(r8 + 1);            // one register ahead (a dead second block: zero records)
            float m[4][4];                                 // m[i][j], xi = 4 i + j; row I is this wave's
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    m[i][j] = i == I ? wino_acc_read(acc[blk * 4 + j][4 * I + t]) : theirs[(((i < I ? i : i - 1) * 16) + j * 4 + t) * 64];
            float s[2][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[0][j] = m[0][j] + m[1][j] + m[2][j];
                s[1][j] = m[1][j] - m[2][j] - m[3][j];
            }
            const auto ws = desc(p.y, r8);
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float y0 = __builtin_fmaf(s[a][0] + s[a][1] + s[a][2], fc[r8], sh[r8]);
                float y1 = __builtin_fmaf(s[a][1] - s[a][2] - s[a][3], fc[r8], sh[r8]);
                const float r0 = rc[2 * a], r1 = rc[2 * a + 1];
                if (p.res_first) { y0 += r0; y1 += r1; }
                y0 = act2d_exact(y0, p.act, p.slope);
                y1 = act2d_exact(y1, p.act, p.slope);
                if (!p.res_first) { y0 += r0; y1 += r1; }
                if (WE) {
                    __builtin_amdgcn_raw_buffer_store_b64((u32x2){__builtin_bit_cast(uint32_t, y0), __builtin_bit_cast(uint32_t, y1)},
                                                          ws, vo[a][0], 0, 0);
                } else {
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, y0), ws, vo[a][0], 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, y1), ws, vo[a][1], 0, 0);
                }
            }
        }
    };
    auto by_row = [&](auto f, int blk) {                   // (wave-uniform)
        if (row == 0) f(std::integral_constant<int, 0>{}, blk);
        else if (row == 1) f(std::integral_constant<int, 1>{}, blk);
        else if (row == 2) f(std::integral_constant<int, 2>{}, blk);
        else f(std::integral_constant<int, 3>{}, blk);
    };
    by_row(xwrite, 0);
    wino_lds_barrier();
    by_row(finish, 0);
    if (live1) {
        wino_lds_barrier();                                // the quad has read block 0
        by_row(xwrite, 1);
        wino_lds_barrier();
        by_row(finish, 1);
    }
}

template <int TWV, bool WE>
__global__ void __launch_bounds__(512, 2) wino3x3_f16x2_pair_kernel(const WinoHP p) {
    constexpr int RW = 32 / TWV;                 // tile rows of a quad; a workgroup is two quads
    constexpr int WGR = 2 * RW;
    constexpr int PR = 2 * WGR + 2;
    constexpr int PC = 2 * TWV + 2;
    constexpr int RS = TWV == 16 ? 48 : 68;
    constexpr int PLANE = PR * RS;
    constexpr int NEL = 8 * PLANE;               // floats of one staged 8-cin image
    constexpr int NDMA = (NEL + 511) / 512;
    constexpr int PBUF = NDMA * 512;
    constexpr int UOFF = 4 * PBUF;               // [2 buffers][2 x 8 cins][PBUF] patches, then 64 records of U (64 KB)
    constexpr int XFLOATS = 2 * 4 * 3 * 16 * 64; // one block's exchange
    static_assert((UOFF + 64 * 256) * 4 <= 160 * 1024 && XFLOATS * 4 <= 160 * 1024, "LDS of a CU");
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const size_t plane_hw = (size_t)p.H * p.W;
    const size_t u_rec = (size_t)p.nblk * 512;           // halves per (chunk, xi, image) record
    const int npair = (p.nblk + 1) >> 1;
    uint32_t voff[NDMA];                          // as in wino3x3_kernel: 0xFFFFFFF0 = outside, the DMA writes 0.0f
    auto fresh_tid = [] {                         // (see wino3x3_f16x2_kernel)
        int t = threadIdx.x;
        asm volatile("" : "+v"(t));
        return t;
    };
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int row = wave & 3, g = wave >> 2;

    // the item: pair of cout blocks, image, first tile; the pairs of one tile block are neighbours in the remapped order
    const uint32_t bid = xcd_remap(blockIdx.x, p.nwg);
    const int nb0 = 2 * (int)(bid % npair);
    const bool live1 = nb0 + 1 < p.nblk;
    uint32_t t = bid / npair;
    const int bx = t % p.wg_tx;
    t /= p.wg_tx;
    const int by = t % p.wg_ty;
    const int b = t / p.wg_ty;
    const int ty0 = by * WGR, tx0 = bx * TWV;
    {
        const int gy0 = 2 * ty0 - 1, gx0 = 2 * tx0 - 1;
        const int lane = fresh_tid() & 63;
#pragma unroll
        for (int i = 0; i < NDMA; ++i) {
            const int e = (wave * NDMA + i) * 64 + lane;
            const int cin = e / PLANE, rem = e - cin * PLANE;
            const int prow = rem / RS, col = rem - prow * RS;
            const int gy = gy0 + prow, gx = gx0 + col;
            const bool ok = e < NEL && col < PC && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W;
            voff[i] = ok ? (uint32_t)((cin * plane_hw + (size_t)gy * p.W + gx) * 4) : 0xFFFFFFF0u;
        }
    }
    auto issue_patch = [&](int c) {
        const float* const xb = p.x + (size_t)b * p.Cin * plane_hw;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // descriptor over channels [16 c + 8 s, Cin) of image b; none left: zero records, every lane reads 0.0f
            const int ch0 = c * 16 + s * 8, left = p.Cin - ch0;
            const auto rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(xb + (size_t)(left > 0 ? ch0 : 0) * plane_hw), 0,
                                                                left > 0 ? (uint32_t)((size_t)left * plane_hw * 4) : 0u, 0x00020000);
            float* pdst = lds + ((c & 1) * 2 + s) * PBUF + wave * NDMA * 64;
#pragma unroll
            for (int i = 0; i < NDMA; ++i)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, pdst + i * 64, 4, voff[i], 0, 0, 0);
        }
    };

    asm volatile("" ::"a"(0.f));                          // AGPR accumulators (see wino3x3_kernel)
    f32x16 acc[8];                                        // [4 blk + j]: position xi = 4 row + j of cout block nb0 + blk

    // the 12 MFMAs of cout block `blk` against its U records 2 (4 row + j) + image; positions in two interleaved pairs so
    // that no MFMA waits on its predecessor
    auto row_m = [&](auto bc, const u32x4* ul, const uint32_t (&vh)[4][4], const uint32_t (&vl)[4][4]) {
        constexpr int BLK = decltype(bc)::value;
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            f16x8 uh[2], ulo[2], us[2], bh[2], bl[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                uh[e] = __builtin_bit_cast(f16x8, ul[(BLK * 32 + 2 * (j + e)) * 64]);
                ulo[e] = __builtin_bit_cast(f16x8, ul[(BLK * 32 + 2 * (j + e) + 1) * 64]);
                us[e] = uh[e] * (_Float16)(1.f / 2048.f);
                bh[e] = __builtin_bit_cast(f16x8, (u32x4){vh[j + e][0], vh[j + e][1], vh[j + e][2], vh[j + e][3]});
                bl[e] = __builtin_bit_cast(f16x8, (u32x4){vl[j + e][0], vl[j + e][1], vl[j + e][2], vl[j + e][3]});
            }
#pragma unroll
            for (int e = 0; e < 2; ++e)
                acc[4 * BLK + j + e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ulo[e], bh[e], acc[4 * BLK + j + e], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 2; ++e)
                acc[4 * BLK + j + e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(us[e], bl[e], acc[4 * BLK + j + e], 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 2; ++e)
                acc[4 * BLK + j + e] = __builtin_amdgcn_mfma_f32_32x32x16_f16(uh[e], bh[e], acc[4 * BLK + j + e], 0, 0, 0);
        }
    };

    issue_patch(0);
    const int lane = fresh_tid() & 63;
    const int li = lane & 31, kk = lane >> 5;
    const int lr = g * RW + li / TWV, lc = li % TWV;
    const int pbase = kk * PBUF + (2 * lr + (row >> 1)) * RS + 2 * lc;
    const u32x4* const ul = (const u32x4*)(lds + UOFF) + (row * 8 * 64 + lane);
    // 64 records of 1 KB, 8 per wave: waves 0-3 bring block nb0, waves 4-7 block nb0 + 1 (if there is one)
    const bool u_live = wave < 4 || live1;
    const uint16_t* const ubase = p.upk + (size_t)(nb0 + (wave >> 2)) * 512 + lane * 8 + (size_t)((wave & 3) * 8) * u_rec;
    auto issue_u = [&](int c) {
        float* udst = lds + UOFF + wave * 8 * 256;
        const uint16_t* usrc = ubase + (size_t)c * 32 * u_rec;
        if (u_live) {
#pragma unroll
            for (int j = 0; j < 8; ++j) __builtin_amdgcn_global_load_lds(usrc + (size_t)j * u_rec, udst + j * 256, 16, 0, 0);
        }
    };
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[k][r] = 0.f;

    __syncthreads();                                       // (vmcnt(0) + barrier: patch 0 has landed)
    // One loop per value of live1 (uniform over the workgroup: all its waves meet the same barriers).  With a branch around
    // the second block's MFMAs inside one loop, hipcc carries that block's 64 accumulator registers through VGPR copies.
    auto k_loop = [&](auto l1) {
        for (int c = 0; c < p.chunks; ++c) {
            issue_u(c);
            if (c + 1 < p.chunks) issue_patch(c + 1);
            const float* pl = lds + (c & 1) * 2 * PBUF + pbase;
            uint32_t vh[4][4], vl[4][4];                   // [position of the row][cin pair]: B fragments, hi and lo' terms
            if (row == 0) wino_row_v<0, 0, PLANE, RS>(pl, vh, vl);
            else if (row == 1) wino_row_v<0, 1, PLANE, RS>(pl, vh, vl);
            else if (row == 2) wino_row_v<1, 0, PLANE, RS>(pl, vh, vl);
            else wino_row_v<1, 1, PLANE, RS>(pl, vh, vl);
            __syncthreads();                               // U of chunk c has landed (vmcnt(0): so has the patch of chunk c + 1)
            row_m(std::integral_constant<int, 0>{}, ul, vh, vl);
            if (decltype(l1)::value) row_m(std::integral_constant<int, 1>{}, ul, vh, vl);
            __syncthreads();                               // every wave is done with U and the patch of chunk c
        }
    };
    if (live1) k_loop(std::true_type{});
    else k_loop(std::false_type{});
    wino_quad_exchange_store<TWV, WE>(p, acc, lds, row, g, fresh_tid() & 63, nb0, live1, b, ty0, tx0);
}

// K10h weight image: fp16 halves [chunk of 16 cins][xi 16][image: 0 hi, 1 lo][cout/32][lane][8], then (cout/32) * 32 floats
// fac[co].  Element j of lane l is cin 16 chunk + 8 (l >> 5) + j of cout 32 blk + (l & 31): the A fragment of
// v_mfma_f32_32x32x16_f16.  U' = 2^k[co] (G g G^T)[xi] scale[co] in float64, rounded to float32; hi = fp16(U'),
// lo = fp16(U' - hi); k[co] puts max |U'| over (cin, xi) into [2^13, 2^14); fac = 2^-(k + kWinoStageExp).
__device__ __forceinline__ double wino_u_f64(const float* g, int xi) {
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    const int a = xi >> 2, bcol = xi & 3;
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int n = 0; n < 3; ++n) s += G[a][m] * (double)g[m * 3 + n] * G[bcol][n];
    return s;
}

__global__ void wino_f16x2_scale_kernel(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ fac,
                                        int cout, int cin, int nblk) {
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= nblk * 32) return;
    double m = 0.0;
    bool bad = false;
    if (co < cout) {
        const double sc = scale != nullptr ? (double)scale[co] : 1.0;
        for (int ci = 0; ci < cin; ++ci)
            for (int xi = 0; xi < 16; ++xi) {
                const double v = fabs(wino_u_f64(w + ((size_t)co * cin + ci) * 9, xi) * sc);
                if (!(v <= 3.0e38)) bad = true;            // Inf, NaN (fmax would drop it) or beyond float32
                m = fmax(m, v);
            }
    }
    int e = 0;
    const bool ok = m > 0.0 && !bad;
    if (ok) frexp(m, &e);                                  // m in [2^(e-1), 2^e)
    const int k = ok ? min(max(14 - e, -100), 100) : 0;
    // a channel with a non-finite weight is marked with a NaN factor: the entry point reads the factors back and refuses
    fac[co] = bad ? __builtin_nanf("") : ldexpf(1.f, -(k + kWinoStageExp));
}

__global__ void wino_pack_f16x2_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                       const float* __restrict__ fac, uint16_t* __restrict__ upk, int cout, int cin, int nblk,
                                       long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int j = i & 7, lane = (i >> 3) & 63;
    long t = i >> 9;
    const int blk = t % nblk; t /= nblk;
    const int img = t & 1, xi = (t >> 1) & 15;
    const int chunk = (int)(t >> 5);
    const int co = blk * 32 + (lane & 31), ci = chunk * 16 + (lane >> 5) * 8 + j;
    float v = 0.f;
    if (co < cout && ci < cin) {
        double s = wino_u_f64(w + ((size_t)co * cin + ci) * 9, xi);
        if (scale != nullptr) s *= (double)scale[co];
        v = (float)(s * (double)(ldexpf(1.f, -kWinoStageExp) / fac[co]));      // 2^k[co]: exact
    }
    const _Float16 hi = (_Float16)v;
    upk[i] = __builtin_bit_cast(uint16_t, img == 0 ? hi : (_Float16)(v - (float)hi));
}

template <int TWV, bool WE, int EXP = 0>
int launch_wino_we(const WinoP& p, hipStream_t st) {
    constexpr int RW = 32 / TWV, PR = 2 * 4 * RW + 2, RS = TWV == 16 ? 48 : 68;
    constexpr int PBUF = (8 * PR * RS + 511) / 512 * 512;
    size_t lds = ((size_t)2 * PBUF + 2 * 16 * 256) * sizeof(float);
    const size_t xchg = (size_t)4 * 2 * 64 * 64 * sizeof(float);          // the pairs' accumulator exchange (128 KB)
    if (lds < xchg) lds = xchg;
    if (occd::ensure_big_lds(reinterpret_cast<const void*>(wino3x3_kernel<TWV, WE, EXP>)) != OCCD_OK) return OCCD_ELAUNCH;
    hipLaunchKernelGGL((wino3x3_kernel<TWV, WE, EXP>), dim3((unsigned)p.nwg), dim3(512), lds, st, p);
    return occd::check_launch();
}

// grid: 0 = one item per workgroup with the single exchange (the earlier kernel); > 0 = that many persistent workgroups
template <int TWV, bool WE>
int launch_wino_f16x2_we(const WinoHP& p, int grid, hipStream_t st) {
    constexpr int RW = 32 / TWV, PR = 2 * 4 * RW + 2, RS = TWV == 16 ? 48 : 68;
    constexpr int PBUF = (8 * PR * RS + 511) / 512 * 512;
    size_t lds = ((size_t)4 * PBUF + 32 * 256) * sizeof(float);
    if (grid > 0) {                                                        // (the 64-KB exchange fits behind patch buffer 0)
        if (occd::ensure_big_lds(reinterpret_cast<const void*>(wino3x3_f16x2_kernel<TWV, true, WE>)) != OCCD_OK) return OCCD_ELAUNCH;
        hipLaunchKernelGGL((wino3x3_f16x2_kernel<TWV, true, WE>), dim3((unsigned)grid), dim3(512), lds, st, p);
        return occd::check_launch();
    }
    const size_t xchg = (size_t)4 * 2 * 64 * 64 * sizeof(float);
    if (lds < xchg) lds = xchg;
    if (occd::ensure_big_lds(reinterpret_cast<const void*>(wino3x3_f16x2_kernel<TWV, false, WE>)) != OCCD_OK) return OCCD_ELAUNCH;
    hipLaunchKernelGGL((wino3x3_f16x2_kernel<TWV, false, WE>), dim3((unsigned)p.nwg), dim3(512), lds, st, p);
    return occd::check_launch();
}

// the cout-pair form: one workgroup per (pair of cout blocks, image, block of 64 tiles)
template <int TWV, bool WE>
int launch_wino_f16x2_pair_we(const WinoHP& p, hipStream_t st) {
    constexpr int RW = 32 / TWV, PR = 2 * 2 * RW + 2, RS = TWV == 16 ? 48 : 68;
    constexpr int PBUF = (8 * PR * RS + 511) / 512 * 512;
    size_t lds = ((size_t)4 * PBUF + 64 * 256) * sizeof(float);
    const size_t xchg = (size_t)2 * 4 * 3 * 16 * 64 * sizeof(float);      // one block's exchange (96 KB)
    if (lds < xchg) lds = xchg;
    if (occd::ensure_big_lds(reinterpret_cast<const void*>(wino3x3_f16x2_pair_kernel<TWV, WE>)) != OCCD_OK) return OCCD_ELAUNCH;
    hipLaunchKernelGGL((wino3x3_f16x2_pair_kernel<TWV, WE>), dim3((unsigned)p.nwg), dim3(512), lds, st, p);
    return occd::check_launch();
}

template <int TWV>
int launch_wino_f16x2_pair(const WinoHP& p, hipStream_t st) {
    return (p.W & 1) == 0 ? launch_wino_f16x2_pair_we<TWV, true>(p, st) : launch_wino_f16x2_pair_we<TWV, false>(p, st);
}

// (even W: the epilogue's 2-pixel accesses, see wino_exchange_store)
template <int TWV, int EXP = 0>
int launch_wino(const WinoP& p, hipStream_t st) {
    return (p.W & 1) == 0 ? launch_wino_we<TWV, true, EXP>(p, st) : launch_wino_we<TWV, false, EXP>(p, st);
}

template <int TWV>
int launch_wino_f16x2(const WinoHP& p, int grid, hipStream_t st) {
    return (p.W & 1) == 0 ? launch_wino_f16x2_we<TWV, true>(p, grid, st) : launch_wino_f16x2_we<TWV, false>(p, grid, st);
}

// Argument checks and launch geometry shared by K10 and K10h (P: WinoP / WinoHP; `cin_step`: cins per chunk).  Returns the
// tile width of a wave pair (16 / 32), or a negative status.
template <class P>
int wino_geometry(const occd_wino_args* a, int cin_step, P& p) {
    if (a == nullptr || a->x == nullptr || a->upk == nullptr || a->y == nullptr) return OCCD_EINVAL;
    if (a->batch < 1 || a->cin < 1 || a->cout < 1 || a->H < 1 || a->W < 1) return OCCD_EINVAL;
    if (a->act < 0 || a->act > 3) return OCCD_EINVAL;
    if ((double)a->cin * a->H * a->W >= 2147483648.0) return OCCD_EINVAL;      // 32-bit offsets inside one image
    if (20.0 * a->H * a->W >= 4294967040.0) return OCCD_EINVAL;                // ... and inside the epilogue's 5 output planes
    p.x = a->x; p.shift = a->shift; p.res = a->res; p.y = a->y;
    p.B = a->batch; p.Cin = a->cin; p.Cout = a->cout; p.H = a->H; p.W = a->W;
    p.chunks = (a->cin + cin_step - 1) / cin_step;
    p.nblk = (a->cout + 31) / 32;
    p.act = a->act; p.res_first = a->res_first; p.slope = a->slope;
    const int th = (a->H + 1) / 2, tw = (a->W + 1) / 2;
    // wide waves (1 x 32 tiles) waste less halo; narrow ones (2 x 16) waste fewer tiles on narrow images
    const int hint = a->tile_hint % 100;
    int twv = hint == 16 || hint == 32 ? hint : 0;
    if (twv == 0) {
        const long w16 = (long)((tw + 15) / 16) * 16 * ((th + 7) / 8) * 8;
        const long w32 = (long)((tw + 31) / 32) * 32 * ((th + 3) / 4) * 4;
        twv = w32 <= w16 ? 32 : 16;
    }
    const int wgr = twv == 16 ? 8 : 4;
    p.wg_tx = (tw + twv - 1) / twv;
    p.wg_ty = (th + wgr - 1) / wgr;
    const long nwg = (long)p.nblk * p.wg_tx * p.wg_ty * p.B;
    if (nwg > 0x7fffffffL) return OCCD_EINVAL;
    p.nwg = (int)nwg;
    return twv;
}

// CUs of the current device (0: unknown), looked up once per device
int wino_cu_count() {
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return 0;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

}  // namespace

extern "C" {

int64_t occd_wino_packed_floats(int32_t cout, int32_t cin) {
    if (cout < 1 || cin < 1) return OCCD_EINVAL;
    return (int64_t)((cin + 7) / 8) * 16 * ((cout + 31) / 32) * 256;
}

int occd_wino_pack_weights(const float* w, const float* scale, float* upk, int32_t cout, int32_t cin, void* stream) {
    if (w == nullptr || upk == nullptr || cout < 1 || cin < 1) return OCCD_EINVAL;
    const long total = occd_wino_packed_floats(cout, cin);
    hipLaunchKernelGGL(wino_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       scale, upk, cout, cin, (cout + 31) / 32, total);
    return occd::check_launch();
}

int occd_wino_conv3x3_fwd(const occd_wino_args* a, void* stream) {
    WinoP p{};
    const int twv = wino_geometry(a, 8, p);
    if (twv < 0) return twv;
    p.upk = a->upk;
    const int th = (a->H + 1) / 2, tw = (a->W + 1) / 2;
    const int exp_mode = a->tile_hint / 100;                  // development switches (see the kernel template)
    const double tiles = (double)p.B * th * tw;
    occd::ProfScope prof("wino_conv3x3", (hipStream_t)stream, 2.0 * 16 * tiles * p.chunks * 8 * p.nblk * 32,
                         4.0 * p.B * ((double)p.Cin + p.Cout) * p.H * p.W);
#ifdef OCCD_WINO_DEV_VARIANTS   // development A/B switches (wrong results by design): not compiled into the library
    if (exp_mode == 1) return twv == 16 ? launch_wino<16, 1>(p, (hipStream_t)stream) : launch_wino<32, 1>(p, (hipStream_t)stream);
    if (exp_mode == 2) return twv == 16 ? launch_wino<16, 2>(p, (hipStream_t)stream) : launch_wino<32, 2>(p, (hipStream_t)stream);
#else
    (void)exp_mode;
#endif
    return twv == 16 ? launch_wino<16>(p, (hipStream_t)stream) : launch_wino<32>(p, (hipStream_t)stream);
}

int64_t occd_wino_packed_f16x2_bytes(int32_t cout, int32_t cin) {
    if (cout < 1 || cin < 1) return OCCD_EINVAL;
    const int64_t nblk = (cout + 31) / 32;
    return (int64_t)((cin + 15) / 16) * 32 * nblk * 512 * 2 + nblk * 32 * 4;
}

int occd_wino_pack_weights_f16x2(const float* w, const float* scale, void* upk, int32_t cout, int32_t cin, void* stream) {
    if (w == nullptr || upk == nullptr || cout < 1 || cin < 1) return OCCD_EINVAL;
    const int nblk = (cout + 31) / 32;
    const long total = (long)((cin + 15) / 16) * 32 * nblk * 512;             // fp16 elements in front of the factors
    float* fac = reinterpret_cast<float*>(static_cast<uint16_t*>(upk) + total);
    hipLaunchKernelGGL(wino_f16x2_scale_kernel, dim3((unsigned)nblk), dim3(32), 0, (hipStream_t)stream, w, scale, fac, cout,
                       cin, nblk);
    hipLaunchKernelGGL(wino_pack_f16x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       scale, fac, static_cast<uint16_t*>(upk), cout, cin, nblk, total);
    const int rc = occd::check_launch();
    if (rc != OCCD_OK) return rc;
    // non-finite weights (times scale) have no power-of-two scale: read the factors back (packing is a set-up step, never
    // part of a captured forward) and refuse; the caller keeps the float32 image of occd_wino_pack_weights
    std::vector<float> host((size_t)nblk * 32);
    if (hipMemcpyAsync(host.data(), fac, host.size() * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return OCCD_ELAUNCH;
    for (float f : host)
        if (f != f) return OCCD_EINVAL;
    return OCCD_OK;
}

int occd_wino_conv3x3_f16x2_fwd_ex(const occd_wino_args* a, int32_t max_workgroups, void* stream) {
    if (max_workgroups < -1) return OCCD_EINVAL;
    WinoHP p{};
    const int twv = wino_geometry(a, 16, p);
    if (twv < 0) return twv;
    p.upk = reinterpret_cast<const uint16_t*>(a->upk);
    p.fac = reinterpret_cast<const float*>(p.upk + (size_t)p.chunks * 32 * p.nblk * 512);
    int grid = 0;                                             // -1: one item per workgroup
    if (max_workgroups > 0) {
        grid = p.nwg < max_workgroups ? p.nwg : max_workgroups;
    } else if (max_workgroups == 0) {
        // one workgroup per CU (LDS allows no more), a multiple of 8 so that a workgroup's items stay on its XCD's slice
        // of the remapped order
        // A launch that gives no workgroup a second item has nothing to hand over and keeps the one-item form: the
        // two-part exchange alone costs it two more barriers (120 items: 0 - 4 % slower, profiles/wino_persist_ab.txt).
        const int cus = wino_cu_count();
        if (cus < 1) return OCCD_ELAUNCH;
        grid = cus >= 8 ? cus - cus % 8 : cus;
        if (p.nwg <= grid) grid = 0;
    }
    const double tiles = (double)p.B * ((a->H + 1) / 2) * ((a->W + 1) / 2);
    // (the algorithmic Winograd-domain flops, K10's figure: the three fp16 MFMAs per product are how they are computed)
    occd::ProfScope prof("wino_conv3x3_f16x2", (hipStream_t)stream, 2.0 * 16 * tiles * ((a->cin + 7) / 8) * 8 * p.nblk * 32,
                         4.0 * p.B * ((double)p.Cin + p.Cout) * p.H * p.W);
    return twv == 16 ? launch_wino_f16x2<16>(p, grid, (hipStream_t)stream) : launch_wino_f16x2<32>(p, grid, (hipStream_t)stream);
}

int occd_wino_conv3x3_f16x2_fwd_form(const occd_wino_args* a, int32_t max_workgroups, int32_t cout_blocks, void* stream) {
    if (cout_blocks != 1 && cout_blocks != 2) return OCCD_EINVAL;
    if (cout_blocks == 1) return occd_wino_conv3x3_f16x2_fwd_ex(a, max_workgroups, stream);
    if (max_workgroups != -1) return OCCD_EINVAL;            // the cout-pair form has no persistent grid
    WinoHP p{};
    const int twv = wino_geometry(a, 16, p);
    if (twv < 0) return twv;
    p.upk = reinterpret_cast<const uint16_t*>(a->upk);
    p.fac = reinterpret_cast<const float*>(p.upk + (size_t)p.chunks * 32 * p.nblk * 512);
    // items of 64 tiles (2 x 32 or 4 x 16) and two cout blocks.  The tile width is still wino_geometry's, which minimises the
    // padding of K10h's 4 x 32 / 8 x 16 workgroups, not of these: correct for any shape, possibly not the faster width (unmeasured)
    const int th = (a->H + 1) / 2, wgr = twv == 16 ? 4 : 2;
    p.wg_ty = (th + wgr - 1) / wgr;
    const long nwg = (long)((p.nblk + 1) / 2) * p.wg_tx * p.wg_ty * p.B;
    if (nwg > 0x7fffffffL) return OCCD_EINVAL;
    p.nwg = (int)nwg;
    const double tiles = (double)p.B * th * ((a->W + 1) / 2);
    // (the tag, flops and bytes of occd_wino_conv3x3_f16x2_fwd_ex: one row of the profile for both forms)
    occd::ProfScope prof("wino_conv3x3_f16x2", (hipStream_t)stream, 2.0 * 16 * tiles * ((a->cin + 7) / 8) * 8 * p.nblk * 32,
                         4.0 * p.B * ((double)p.Cin + p.Cout) * p.H * p.W);
    return twv == 16 ? launch_wino_f16x2_pair<16>(p, (hipStream_t)stream) : launch_wino_f16x2_pair<32>(p, (hipStream_t)stream);
}

int occd_wino_conv3x3_f16x2_fwd(const occd_wino_args* a, void* stream) {
    // OCCDEPTH_WINO_PERSIST: unset or "0" = one workgroup per item, "1" = persistent; anything else is refused, as in hip.py
    static const int dflt = [] {
        const char* e = getenv("OCCDEPTH_WINO_PERSIST");
        if (e == nullptr || (e[0] == '0' && e[1] == '\0')) return -1;
        return e[0] == '1' && e[1] == '\0' ? 0 : -2;
    }();
    if (dflt < -1) return OCCD_EINVAL;
    return occd_wino_conv3x3_f16x2_fwd_ex(a, dflt, stream);
}

}  // extern "C"
