// The Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) on the K38 sort (csrc/sort.hip): the convex surrogate of the
// per-class Jaccard index, over the whole batch and the classes present in the target.
//   occd_lovasz_errors  one streaming voxel pass: softmax, then per class a sort key (a monotone map of the float32 bits of
//                       the error e, descending e = ascending key) and a payload (voxel index, fg flag in bit 31) into
//                       that class's segment
//   occd_lovasz_ranks   along each SORTED segment: an inclusive scan of the fg flag in three launches (tile sums, one scan
//                       of the sums per segment, apply -- no workgroup waits for another), then per element the
//                       closed-form Jaccard increment g in float64 from the integer counters, e g into L_c (Q60, integer
//                       atomics) and the signed g into the voxel-major table q (N, C)
//   occd_lovasz_bwd     one streaming voxel pass: recomputes p, reads q, writes d L / d logits in the logits' own layout
// L_c and q are sums and functions of integers: loss and gradient are bitwise reproducible whatever the schedule.  No
// allocation, no host sync, no memset node: capture-safe.  Contract, and the rounding bound of L_c: include/occdepth_amd.h.
#include "common.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kMaxC = 32;
constexpr u32 kOneBits = 0x3F800000u;              // the float32 bits of 1.0f
constexpr u32 kInvalid = OCCD_LOVASZ_INVALID_KEY;
constexpr int kRankTile = OCCD_LOVASZ_RANK_TILE;
constexpr int kRankItems = kRankTile / 256;        // consecutive elements per thread
constexpr double kQ = (double)((u64)1 << OCCD_LOVASZ_Q);
static_assert(kInvalid > kOneBits && kInvalid < (1u << OCCD_LOVASZ_KEY_BITS), "the sentinel sorts behind every error");

struct LP {
    const float* logits;
    const uint8_t* target;
    u32* keys;
    u32* vals;
    u32* tsum;
    float* q;
    u64* fg_count;
    u64* loss_q;
    const float* gscale;
    float* grad;
    long total;                // N = B * S
    long S;
    long s_b, s_c, s_v, g_b, g_c, g_v;
    int C, c0, cc, g_pad, ignore;
    u32 tiles;
};

// probabilities of one voxel, p[] statically indexed (the class bucket CB >= C); expf: the loss is held to a float64
// restatement (render_loss.hip's helper restated: the sources of the existing kernels stay what they were)
template <int CB>
__device__ __forceinline__ void softmax_regs(const float* lp, int C, long s_c, float (&p)[CB]) {
    if (s_c == 1) {
#pragma unroll
        for (int c4 = 0; c4 < CB; c4 += 4)
            if (c4 < C) {
                const float4 v = *(const float4*)(lp + c4);
                p[c4] = v.x;
                if (c4 + 1 < CB) p[c4 + 1] = v.y;
                if (c4 + 2 < CB) p[c4 + 2] = v.z;
                if (c4 + 3 < CB) p[c4 + 3] = v.w;
            }
    } else {
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (c < C) p[c] = lp[(size_t)c * s_c];
    }
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) m = fmaxf(m, p[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) {
            p[c] = expf(p[c] - m);
            sum += p[c];
        }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < CB; ++c)
        if (c < C) p[c] *= inv;
}

template <int CB>
__global__ void __launch_bounds__(256) errors_kernel(const LP q) {
    const int C = q.C;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < q.total; v += (long)gridDim.x * 256) {
        const int y = q.target[v];
        const bool known = y != q.ignore;
        float p[CB];
        if (known) {
            const long b = v / q.S;
            const long s = v - b * q.S;
            softmax_regs<CB>(q.logits + (size_t)b * q.s_b + (size_t)s * q.s_v, C, q.s_c, p);
            // the foreground class's error 1 - p_y as the sum of the others: a saturated voxel gives an exact 0
            float others = 0.f;
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C && c != y) others += p[c];
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c == y) p[c] = others;
        }
#pragma unroll
        for (int c = 0; c < CB; ++c) {
            const int j = c - q.c0;
            if (c < C && j >= 0 && j < q.cc) {
                u32 key = kInvalid, val = (u32)v;
                if (known) {
                    const float e = fminf(fmaxf(p[c], 0.f), 1.f);    // NaN -> 0
                    key = kOneBits - __float_as_uint(e);
                    if (c == y) val |= 0x80000000u;
                }
                q.keys[(size_t)j * q.total + v] = key;
                q.vals[(size_t)j * q.total + v] = val;
            }
        }
    }
}

// the foreground flags of a tile, summed
__global__ void __launch_bounds__(256) fg_sum_kernel(const LP q) {
    __shared__ u32 sh;
    if (threadIdx.x == 0) sh = 0;
    __syncthreads();
    const u32 tile = blockIdx.x, seg = blockIdx.y;
    const u32* vals = q.vals + (size_t)seg * q.total;
    const long t0 = (long)tile * kRankTile;
    u32 n = 0;
#pragma unroll
    for (int j = 0; j < kRankItems; ++j) {
        const long i = t0 + j * 256 + threadIdx.x;
        if (i < q.total) n += vals[i] >> 31;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&sh, n);
    __syncthreads();
    if (threadIdx.x == 0) q.tsum[(size_t)seg * q.tiles + tile] = sh;
}

// one workgroup per segment: exclusive scan of the tile sums in place; G_c; L_c <- 0
__global__ void __launch_bounds__(1024) fg_scan_kernel(const LP q) {
    __shared__ u32 wsum[16];
    __shared__ u32 carry_sh;
    const u32 seg = blockIdx.x;
    u32* t = q.tsum + (size_t)seg * q.tiles;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 carry = 0;
    for (u32 base = 0; base < q.tiles; base += 1024) {
        const u32 i = base + threadIdx.x;
        const u32 v = i < q.tiles ? t[i] : 0u;
        u32 inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 x = __shfl_up(inc, o);
            if (lane >= o) inc += x;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u32 before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (threadIdx.x == 1023) carry_sh = before + inc;
        if (i < q.tiles) t[i] = before + inc - v;
        __syncthreads();
        carry = carry_sh;
    }
    if (threadIdx.x == 0) {
        q.fg_count[q.c0 + seg] = carry;
        q.loss_q[q.c0 + seg] = 0;
    }
}

__global__ void __launch_bounds__(256) apply_kernel(const LP q) {
    __shared__ u32 wsum[4];
    __shared__ u64 lsum;
    const u32 tile = blockIdx.x, seg = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) lsum = 0;
    const u32* keys = q.keys + (size_t)seg * q.total;
    const u32* vals = q.vals + (size_t)seg * q.total;
    const long G = (long)q.fg_count[q.c0 + seg];                     // written by the scan launch before this one
    const long i0 = (long)tile * kRankTile + (long)threadIdx.x * kRankItems;
    u32 key[kRankItems], val[kRankItems];
    u32 sum = 0;
#pragma unroll
    for (int j = 0; j < kRankItems; ++j) {
        const bool in = i0 + j < q.total;
        key[j] = in ? keys[i0 + j] : kInvalid;
        val[j] = in ? vals[i0 + j] : 0u;
        sum += val[j] >> 31;
    }
    u32 inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 x = __shfl_up(inc, o);
        if (lane >= o) inc += x;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long Fi = (long)q.tsum[(size_t)seg * q.tiles + tile] + inc - sum;   // #fg before this thread's first element
    for (int w = 0; w < wave; ++w) Fi += wsum[w];
    u64 acc = 0;
#pragma unroll
    for (int j = 0; j < kRankItems; ++j) {
        if (key[j] >= kInvalid) continue;                              // unknown voxels (all behind the valid ones), the tail
        const bool fg = val[j] >> 31;
        const long F = Fi;                                             // #fg strictly before
        Fi += fg;
        const long b = (i0 + j + 1) - Fi;                              // #bg up to and including this one
        double g = 0.0;
        if (G > 0) g = fg ? 1.0 / (double)(G + b) : (double)(G - F) / ((double)(G + b - 1) * (double)(G + b));
        const float e = __uint_as_float(kOneBits - key[j]);
        acc += (u64)__double2ll_rn((double)e * g * kQ);
        const float gf = (float)g;
        const u32 voxel = val[j] & 0x7fffffffu;
        if (voxel < q.total) q.q[(size_t)voxel * q.C + q.c0 + seg] = fg ? -gf : gf;   // a payload is trusted only in range
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
    if (lane == 0 && acc) atomicAdd(&lsum, acc);
    __syncthreads();
    if (threadIdx.x == 0 && lsum) atomicAdd(&q.loss_q[q.c0 + seg], lsum);
}

template <int CB>
__global__ void __launch_bounds__(256) bwd_kernel(const LP q) {
    const float gs = q.gscale[0];
    const int C = q.C;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < q.total; v += (long)gridDim.x * 256) {
        const long b = v / q.S;
        const long s = v - b * q.S;
        float p[CB];
        if (q.target[v] != q.ignore) {
            softmax_regs<CB>(q.logits + (size_t)b * q.s_b + (size_t)s * q.s_v, C, q.s_c, p);
            const float* qr = q.q + (size_t)v * C;
            float qv[CB];
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) {
                    qv[c] = qr[c];
                    dot += qv[c] * p[c];
                }
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) p[c] = gs * (p[c] * (qv[c] - dot));
        } else {
#pragma unroll
            for (int c = 0; c < CB; ++c) p[c] = 0.f;
        }
        float* gp = q.grad + (size_t)b * q.g_b + (size_t)s * q.g_v;
        if (q.g_c == 1) {
            // channels-last gradient rows: 16-byte stores, pad channels [C, g_pad) written as zeros
            constexpr int CB4 = (CB + 3) & ~3;
            float o[CB4];
#pragma unroll
            for (int c = 0; c < CB4; ++c) o[c] = 0.f;
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) o[c] = p[c];
#pragma unroll
            for (int c4 = 0; c4 < CB4; c4 += 4)
                if (c4 < q.g_pad) *(float4*)(gp + c4) = float4{o[c4], o[c4 + 1], o[c4 + 2], o[c4 + 3]};
            for (int c = CB4; c < q.g_pad; ++c) gp[c] = 0.f;
        } else {
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) gp[(size_t)c * q.g_c] = p[c];
        }
    }
}

int grid_for(long total) {
    long blocks = (total + 255) / 256;
    const long cap = 256 * 8;
    return (int)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

// (B, C, S) planes or channels-last rows, as the strided ssc-loss kernels take them
bool strides_ok(const float* base, int32_t C, int64_t s_b, int64_t s_c, int64_t s_v) {
    if (s_c == 1) return s_v >= C && (s_v & 3) == 0 && (s_b & 3) == 0 && ((uintptr_t)base & 15) == 0;
    return s_v >= 1 && s_c >= 1 && s_b >= 0;
}

bool volume_ok(const OccdLovaszArgs* a) {
    if (a->batch <= 0 || a->S <= 0 || a->S >= ((int64_t)1 << 31)) return false;
    if ((int64_t)a->batch * a->S >= ((int64_t)1 << 31)) return false;
    return a->C >= 2 && a->C <= kMaxC && a->c0 >= 0 && a->cc >= 1 && a->c0 + a->cc <= a->C;
}

bool logits_ok(const OccdLovaszArgs* a) {
    return a->logits != nullptr && a->target != nullptr && strides_ok(a->logits, a->C, a->s_b, a->s_c, a->s_v);
}

void fill(LP& q, const OccdLovaszArgs* a) {
    q.logits = a->logits; q.target = a->target; q.keys = a->keys; q.vals = a->vals; q.tsum = a->tsum; q.q = a->q;
    q.fg_count = (u64*)a->fg_count; q.loss_q = (u64*)a->loss_q; q.gscale = a->gscale; q.grad = a->grad;
    q.S = a->S; q.total = (long)a->batch * a->S;
    q.s_b = a->s_b; q.s_c = a->s_c; q.s_v = a->s_v; q.g_b = a->g_b; q.g_c = a->g_c; q.g_v = a->g_v;
    q.C = a->C; q.c0 = a->c0; q.cc = a->cc; q.g_pad = a->g_pad; q.ignore = a->ignore;
    q.tiles = (u32)((q.total + kRankTile - 1) / kRankTile);
}

}  // namespace

extern "C" int occd_lovasz_errors(const OccdLovaszArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !logits_ok(a) || !a->keys || !a->vals) return OCCD_EINVAL;
    LP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("lovasz_errors", st, (double)q.total * a->C * 4.0, (double)q.total * (4.0 * a->C + 1.0 + 8.0 * a->cc));
    const dim3 grid(grid_for(q.total));
    if (a->C <= 4) hipLaunchKernelGGL(errors_kernel<4>, grid, dim3(256), 0, st, q);
    else if (a->C <= 12) hipLaunchKernelGGL(errors_kernel<12>, grid, dim3(256), 0, st, q);
    else if (a->C <= 20) hipLaunchKernelGGL(errors_kernel<20>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(errors_kernel<32>, grid, dim3(256), 0, st, q);
    return occd::check_launch();
}

extern "C" int occd_lovasz_ranks(const OccdLovaszArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !a->keys || !a->vals || !a->tsum || !a->q || !a->fg_count || !a->loss_q) return OCCD_EINVAL;
    LP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    const double pairs = (double)q.total * a->cc;
    occd::ProfScope prof("lovasz_ranks", st, pairs * 4.0, pairs * 16.0);
    const dim3 grid(q.tiles, (unsigned)a->cc);
    hipLaunchKernelGGL(fg_sum_kernel, grid, dim3(256), 0, st, q);
    hipLaunchKernelGGL(fg_scan_kernel, dim3((unsigned)a->cc), dim3(1024), 0, st, q);
    hipLaunchKernelGGL(apply_kernel, grid, dim3(256), 0, st, q);
    return occd::check_launch();
}

extern "C" int occd_lovasz_bwd(const OccdLovaszArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !logits_ok(a) || !a->q || !a->gscale || !a->grad) return OCCD_EINVAL;
    if (!strides_ok(a->grad, a->C, a->g_b, a->g_c, a->g_v)) return OCCD_EINVAL;
    if (a->g_c == 1 ? (a->g_pad < a->C || a->g_pad > a->g_v || (a->g_pad & 3)) : a->g_pad != 0) return OCCD_EINVAL;
    LP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("lovasz_bwd", st, (double)q.total * a->C * 6.0, (double)q.total * (12.0 * a->C + 1.0));
    const dim3 grid(grid_for(q.total));
    if (a->C <= 4) hipLaunchKernelGGL(bwd_kernel<4>, grid, dim3(256), 0, st, q);
    else if (a->C <= 12) hipLaunchKernelGGL(bwd_kernel<12>, grid, dim3(256), 0, st, q);
    else if (a->C <= 20) hipLaunchKernelGGL(bwd_kernel<20>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(bwd_kernel<32>, grid, dim3(256), 0, st, q);
    return occd::check_launch();
}
