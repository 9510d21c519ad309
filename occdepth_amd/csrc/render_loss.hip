// K36: depth-rendering loss.  The soft occupancy of the logits is alpha-composited along the left camera's pixel rays into
// an expected depth image, which is held to a metric depth map; forward and backward, four kernels:
//   occd_render_opacity          z -> a = 1 - softmax(z)[0] = sum_{c > 0} p_c, (B, S) float32 (signed form), one streaming pass
//   occd_render_depth_fwd        one thread per ray: d^ = sum_i T_i a_i t_i + T_{n+1} t_end, opacity 1 - T_{n+1}, loss sums
//   occd_render_depth_bwd_rays   the same walk again: per visited voxel one 64-bit integer atomic into H (B, S), Q32
//   occd_render_depth_bwd_voxels streaming: d L / d z_{v,c} = gscale H_v p_c (c > 0), -gscale H_v a_v (c = 0); H_v <- 0
// Every ray pass gathers 4 bytes per step (the opacity) instead of C logits and C exponentials.  A wave is an 8 x 8 tile of
// neighbouring rays (render.hip's tiling), so its gathers fall into few cache lines.  The loss sum (Q24) and H (Q32) are
// integers added with integer atomics: the loss and the gradient are bitwise reproducible whatever the schedule.  No
// allocation, no host sync, no memset node: capture-safe.  Contract: include/occdepth_amd.h.
//
// The walk is occd_render_voxels' (csrc/raycast.h) restated: the same float32 expressions in the same order, so that with
// hard logits (a = 0 or 1 exactly) d^ is, bit for bit, the depth that kernel reports.  Like render.hip this kernel does
// not take them from raycast.h: on the header its forward pass measured 1.7 - 1.9 % slower at every stride, with the loop
// written out as well as through a callback (profiles/raycast_refactor.txt).  A change to the walk is made there and here.
#include "common.h"

namespace {

constexpr int kMaxC = 32;
constexpr int kTile = 8;                   // a wave's ray tile is kTile x kTile
constexpr int kBlockW = 16, kBlockH = 16;  // 4 waves = 2 x 2 tiles per workgroup
constexpr double kQ24 = 16777216.0;
constexpr double kQ32 = 4294967296.0;
constexpr float kRelFloor = 0.25f;         // rel: omega = 1 / max(D_r, kRelFloor), so |omega term| <= 2^9 and |H| < 2^62
typedef unsigned long long u64;

struct RLP {
    const float* logits;
    float* opacity;
    const float* views;
    const float* gt;
    float* depth;
    float* alpha;
    u64* stats;
    u64* hsum;
    const float* gscale;
    float* grad;
    long total;                // B * S
    long s_b, s_c, s_v, g_b, g_c, g_v;
    long d_b, d_h, d_w;
    int C, S, g_pad;
    int X, Y, Z, H, W, h, w, stride, off_u, off_v, norm;
    float max_depth;
};

// probabilities of one voxel, p[] statically indexed (the class bucket CB >= C); expf, not __expf: the opacity is held to
// a float64 restatement
template <int CB>
__device__ __forceinline__ void softmax_regs(const float* lp, int C, long s_c, float (&p)[CB]) {
    if (s_c == 1) {
        // channels-last row: 16-byte loads (rows are 16-byte aligned and padded to a multiple of 4 floats)
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

// a = sum_{c > 0} p_c: no cancellation when p_0 -> 1
template <int CB>
__device__ __forceinline__ float opacity_of(const float (&p)[CB], int C) {
    float a = 0.f;
#pragma unroll
    for (int c = 1; c < CB; ++c)
        if (c < C) a += p[c];
    return fminf(a, 1.f);                  // the sum of rounded quotients can exceed 1 by an ulp
}

template <int CB>
__global__ void __launch_bounds__(256) opacity_kernel(const RLP q) {
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < q.total; v += (long)gridDim.x * 256) {
        const long b = v / q.S;
        const int s = (int)(v - b * q.S);
        float p[CB];
        softmax_regs<CB>(q.logits + (size_t)b * q.s_b + (size_t)s * q.s_v, q.C, q.s_c, p);
        // 4 bytes that keep the relative precision of BOTH a and 1 - a: a itself up to 1/2, -p_0 above (the sign bit says
        // which).  1 - a formed from a float32 a near 1 would carry ulp(1) / (1 - a) of relative error into every
        // transmittance behind the voxel and into its own gradient.  p_0 < 2^-25: a rounds to 1, the voxel is opaque (-0.0f).
        const float a = opacity_of<CB>(p, q.C);
        q.opacity[v] = a <= 0.5f ? a : (p[0] >= 0x1p-25f ? -p[0] : -0.f);
    }
}

template <int CB>
__global__ void __launch_bounds__(256) bwd_voxels_kernel(const RLP q) {
    const float gs = q.gscale[0];
    const int C = q.C;
    for (long v = (long)blockIdx.x * 256 + threadIdx.x; v < q.total; v += (long)gridDim.x * 256) {
        const long b = v / q.S;
        const int s = (int)(v - b * q.S);
        const long long hq = (long long)q.hsum[v];
        float p[CB];
        if (hq != 0) {
            softmax_regs<CB>(q.logits + (size_t)b * q.s_b + (size_t)s * q.s_v, C, q.s_c, p);
            q.hsum[v] = 0;                 // H is clean after every backward
            const float a = opacity_of<CB>(p, C);
            const float hv = gs * (float)((double)hq * (1.0 / kQ32));
            p[0] = -a;
#pragma unroll
            for (int c = 0; c < CB; ++c)
                if (c < C) p[c] *= hv;
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

__global__ void zero2_kernel(u64* p) {
    if (threadIdx.x < 2) p[threadIdx.x] = 0;
}

// BWD = false: the forward ray pass; BWD = true: the backward ray pass (reads d^ back, adds into H)
template <bool BWD>
__global__ __launch_bounds__(kBlockW * kBlockH) void ray_kernel(const RLP p) {
#pragma clang fp contract(off)   // every product and sum rounds once: tests/test_render_loss.py restates this arithmetic in numpy
    __shared__ u64 sh[2];
    if (!BWD) {
        if (threadIdx.x < 2) sh[threadIdx.x] = 0;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kBlockW + (wave & 1) * kTile + (lane & 7);       // ray column
    const int j = blockIdx.y * kBlockH + (wave >> 1) * kTile + (lane >> 3);     // ray row
    const int b = blockIdx.z;
    u64 loss = 0, cnt = 0;
    if (i < p.w && j < p.h) {
        const int u = p.off_u + p.stride * i, v = p.off_v + p.stride * j;       // the pixel: u < W, v < H by h, w
        const int64_t ray = ((int64_t)b * p.h + j) * p.w + i;
        const int X = p.X, Y = p.Y, Z = p.Z;
        const float* g = p.views + (int64_t)b * 18;
        const float fu = (float)u + 0.5f, fv = (float)v + 0.5f;
        const float ox = g[0] + fu * g[3] + fv * g[6], oy = g[1] + fu * g[4] + fv * g[7], oz = g[2] + fu * g[5] + fv * g[8];
        const float dx = g[9] + fu * g[12] + fv * g[15], dy = g[10] + fu * g[13] + fv * g[16],
                    dz = g[11] + fu * g[14] + fv * g[17];
        const float inf = __builtin_inff();
        const float fX = (float)X, fY = (float)Y, fZ = (float)Z;
        bool alive = (ox - ox) + (oy - oy) + (oz - oz) + (dx - dx) + (dy - dy) + (dz - dz) == 0.f;   // all finite
        // slab test; a zero component is parallel: inside or outside by the origin, never a division
        float tn = -inf, tf = inf, t = 0.f;
        const float ix_ = dx != 0.f ? 1.f / dx : 0.f, iy_ = dy != 0.f ? 1.f / dy : 0.f, iz_ = dz != 0.f ? 1.f / dz : 0.f;
        if (dx != 0.f) {
            const float a = (0.f - ox) * ix_, c = (fX - ox) * ix_;
            const float n = fminf(a, c);
            if (n > tn) tn = n;
            tf = fminf(tf, fmaxf(a, c));
        } else if (!(ox >= 0.f && ox < fX)) alive = false;
        if (dy != 0.f) {
            const float a = (0.f - oy) * iy_, c = (fY - oy) * iy_;
            const float n = fminf(a, c);
            if (n > tn) tn = n;
            tf = fminf(tf, fmaxf(a, c));
        } else if (!(oy >= 0.f && oy < fY)) alive = false;
        if (dz != 0.f) {
            const float a = (0.f - oz) * iz_, c = (fZ - oz) * iz_;
            const float n = fminf(a, c);
            if (n > tn) tn = n;
            tf = fminf(tf, fmaxf(a, c));
        } else if (!(oz >= 0.f && oz < fZ)) alive = false;
        if (tn > 0.f) t = tn;
        if (!(tf >= t)) alive = false;
        const float t_entry = t;
        const float t_end = alive ? fminf(tf, p.max_depth) : p.max_depth;     // a ray that misses the grid renders empty
        // the target: D finite, 0 < D <= max_depth, behind the grid's entry; a surface behind the exit asks for an empty ray
        bool valid = false;
        float Dr = 0.f, omega = 0.f;
        if (p.gt != nullptr) {
            const float D = p.gt[(int64_t)b * p.d_b + (int64_t)v * p.d_h + (int64_t)u * p.d_w];
            valid = alive && (D - D == 0.f) && D > 0.f && D <= p.max_depth && D > t_entry;
            Dr = fminf(D, t_end);
            omega = p.norm ? 1.f / fmaxf(Dr, kRelFloor) : 1.f;
        }
        float dhat = 0.f, sgn = 0.f;
        if (BWD) {
            dhat = p.depth[ray];
            sgn = dhat > Dr ? omega : dhat < Dr ? -omega : 0.f;                // omega sign(d^ - D_r), sign(0) = 0
        }
        float T = 1.f, acc = 0.f;
        if (alive && t < p.max_depth && (!BWD || (valid && sgn != 0.f))) {
            // first voxel, clamped as floats so that the conversion is always in range
            int ix = (int)fminf(fmaxf(floorf(ox + dx * t), 0.f), fX - 1.f);
            int iy = (int)fminf(fmaxf(floorf(oy + dy * t), 0.f), fY - 1.f);
            int iz = (int)fminf(fmaxf(floorf(oz + dz * t), 0.f), fZ - 1.f);
            const int sx = dx > 0.f ? 1 : dx < 0.f ? -1 : 0, sy = dy > 0.f ? 1 : dy < 0.f ? -1 : 0,
                      sz = dz > 0.f ? 1 : dz < 0.f ? -1 : 0;
            // t at which the ray leaves the current voxel along each axis, from the boundary itself (no running sum)
            float mx = sx ? ((float)(ix + (sx > 0)) - ox) * ix_ : inf;
            float my = sy ? ((float)(iy + (sy > 0)) - oy) * iy_ : inf;
            float mz = sz ? ((float)(iz + (sz > 0)) - oz) * iz_ : inf;
            const int64_t frame = (int64_t)b * X * Y * Z;
            const int steps = X + Y + Z + 3;          // every step moves one index one way: at most X + Y + Z - 2 in range
            for (int n = 0; n < steps; ++n) {
                const int vox = (ix * Y + iy) * Z + iz;           // 0 <= ix < X, ... holds here, always: vox < X Y Z
                const float s = p.opacity[frame + vox];           // a, or -(1 - a) behind the sign bit (occd_render_opacity)
                const bool comp = __float_as_int(s) < 0;
                const float a = comp ? 1.f + s : s;
                const float wt = T * a;
                acc = acc + wt * t;                               // pre_k
                T = T * (comp ? -s : 1.f - s);                    // T_{k+1}
                if (BWD) {
                    // d d^ / d a_k (1 - a_k) = T_{k+1} t_k - (d^ - pre_k); zero contributions are skipped
                    const float term = (T * t - (dhat - acc)) * sgn;
                    const long long hq = __double2ll_rn((double)term * kQ32);
                    if (hq != 0) atomicAdd(&p.hsum[frame + vox], (u64)hq);
                }
                if (T == 0.f) break;                              // everything behind is weighted by an exact zero
                // the nearest boundary, x before y before z on ties
                const int ax = (mx <= my && mx <= mz) ? 0 : (my <= mz) ? 1 : 2;
                const float m = ax == 0 ? mx : ax == 1 ? my : mz;
                if (!(m < p.max_depth)) break;                    // the next voxel is entered at or past max_depth (or never)
                if (ax == 0) {
                    ix += sx;
                    if (ix < 0 || ix >= X) break;
                    mx = ((float)(ix + (sx > 0)) - ox) * ix_;
                } else if (ax == 1) {
                    iy += sy;
                    if (iy < 0 || iy >= Y) break;
                    my = ((float)(iy + (sy > 0)) - oy) * iy_;
                } else {
                    iz += sz;
                    if (iz < 0 || iz >= Z) break;
                    mz = ((float)(iz + (sz > 0)) - oz) * iz_;
                }
                t = m;
            }
        }
        if (!BWD) {
            dhat = acc + T * t_end;
            p.depth[ray] = dhat;
            p.alpha[ray] = 1.f - T;
            if (valid) {
                loss = (u64)((double)(omega * fabsf(dhat - Dr)) * kQ24 + 0.5);
                cnt = 1;
            }
        }
    }
    if (!BWD) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            loss += __shfl_down(loss, o);
            cnt += __shfl_down(cnt, o);
        }
        if ((threadIdx.x & 63) == 0) {
            if (loss) atomicAdd(&sh[0], loss);
            if (cnt) atomicAdd(&sh[1], cnt);
        }
        __syncthreads();
        if (p.stats != nullptr && threadIdx.x < 2 && sh[threadIdx.x]) atomicAdd(&p.stats[threadIdx.x], sh[threadIdx.x]);
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

bool volume_ok(const OccdRenderLossArgs* a) {
    if (a->batch <= 0 || a->batch > 256 || a->X <= 0 || a->Y <= 0 || a->Z <= 0) return false;
    const int64_t xy = (int64_t)a->X * a->Y;
    return xy < ((int64_t)1 << 31) && xy * a->Z < ((int64_t)1 << 31) && (int64_t)a->batch * xy * a->Z < ((int64_t)1 << 40);
}

bool logits_ok(const OccdRenderLossArgs* a) {
    return a->logits != nullptr && a->C >= 2 && a->C <= kMaxC && strides_ok(a->logits, a->C, a->s_b, a->s_c, a->s_v);
}

// the image of rays: h = ceil((H - off_v) / stride), w = ceil((W - off_u) / stride), at most 2^21 rays per frame (the
// bound of H: |term| <= 2^9 in Q32 over 2^21 rays stays below 2^62)
bool rays_ok(const OccdRenderLossArgs* a) {
    if (a->views == nullptr || a->opacity == nullptr || a->depth == nullptr) return false;
    if (a->H <= 0 || a->W <= 0 || a->stride <= 0 || a->off_u < 0 || a->off_v < 0 || a->off_u >= a->stride || a->off_v >= a->stride)
        return false;
    if (a->off_u >= a->W || a->off_v >= a->H) return false;
    if (a->h != (a->H - a->off_v + a->stride - 1) / a->stride || a->w != (a->W - a->off_u + a->stride - 1) / a->stride) return false;
    if ((int64_t)a->h * a->w > ((int64_t)1 << 21) || (a->h + kBlockH - 1) / kBlockH > 65535) return false;
    if (!(a->max_depth > 0.f && a->max_depth <= 128.f)) return false;
    if (a->norm != OCCD_RENDER_LOSS_ABS && a->norm != OCCD_RENDER_LOSS_REL) return false;
    if (a->gt_depth != nullptr && (a->d_b < 0 || a->d_h < 0 || a->d_w < 0)) return false;
    return true;
}

void fill(RLP& q, const OccdRenderLossArgs* a) {
    q.logits = a->logits; q.opacity = a->opacity; q.views = a->views; q.gt = a->gt_depth; q.depth = a->depth;
    q.alpha = a->alpha; q.stats = (u64*)a->stats; q.hsum = (u64*)a->hsum; q.gscale = a->gscale; q.grad = a->grad;
    q.S = a->X * a->Y * a->Z; q.total = (long)a->batch * q.S;
    q.s_b = a->s_b; q.s_c = a->s_c; q.s_v = a->s_v; q.g_b = a->g_b; q.g_c = a->g_c; q.g_v = a->g_v; q.g_pad = a->g_pad;
    q.d_b = a->d_b; q.d_h = a->d_h; q.d_w = a->d_w;
    q.C = a->C; q.X = a->X; q.Y = a->Y; q.Z = a->Z; q.H = a->H; q.W = a->W; q.h = a->h; q.w = a->w;
    q.stride = a->stride; q.off_u = a->off_u; q.off_v = a->off_v; q.norm = a->norm; q.max_depth = a->max_depth;
}

dim3 ray_grid(const OccdRenderLossArgs* a) {
    return dim3((unsigned)((a->w + kBlockW - 1) / kBlockW), (unsigned)((a->h + kBlockH - 1) / kBlockH), (unsigned)a->batch);
}

}  // namespace

extern "C" int occd_render_opacity(const OccdRenderLossArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !logits_ok(a) || !a->opacity) return OCCD_EINVAL;
    RLP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("render_opacity", st, (double)q.total * a->C * 4.0, (double)q.total * (4.0 * a->C + 4.0));
    const dim3 grid(grid_for(q.total));
    if (a->C <= 4) hipLaunchKernelGGL(opacity_kernel<4>, grid, dim3(256), 0, st, q);
    else if (a->C <= 12) hipLaunchKernelGGL(opacity_kernel<12>, grid, dim3(256), 0, st, q);
    else if (a->C <= 20) hipLaunchKernelGGL(opacity_kernel<20>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(opacity_kernel<32>, grid, dim3(256), 0, st, q);
    return occd::check_launch();
}

extern "C" int occd_render_depth_fwd(const OccdRenderLossArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !rays_ok(a) || !a->alpha) return OCCD_EINVAL;
    if ((a->gt_depth != nullptr) != (a->stats != nullptr)) return OCCD_EINVAL;       // a target and its sums come together
    RLP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    // the sums are zeroed with a kernel, not a memset node (see occd_ssc_loss_stats_fwd_strided)
    if (a->stats) hipLaunchKernelGGL(zero2_kernel, dim3(1), dim3(64), 0, st, q.stats);
    const double rays = (double)a->batch * a->h * a->w;
    occd::ProfScope prof("render_depth_fwd", st, 0.0, (double)q.total * 4.0 + rays * (a->gt_depth ? 12.0 : 8.0));
    hipLaunchKernelGGL(ray_kernel<false>, ray_grid(a), dim3(kBlockW * kBlockH), 0, st, q);
    return occd::check_launch();
}

extern "C" int occd_render_depth_bwd_rays(const OccdRenderLossArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !rays_ok(a) || !a->gt_depth || !a->hsum) return OCCD_EINVAL;
    RLP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    const double rays = (double)a->batch * a->h * a->w;
    occd::ProfScope prof("render_depth_bwd_rays", st, 0.0, (double)q.total * 12.0 + rays * 8.0);
    hipLaunchKernelGGL(ray_kernel<true>, ray_grid(a), dim3(kBlockW * kBlockH), 0, st, q);
    return occd::check_launch();
}

extern "C" int occd_render_depth_bwd_voxels(const OccdRenderLossArgs* a, void* stream) {
    if (!a || !volume_ok(a) || !logits_ok(a) || !a->hsum || !a->gscale || !a->grad) return OCCD_EINVAL;
    if (!strides_ok(a->grad, a->C, a->g_b, a->g_c, a->g_v)) return OCCD_EINVAL;
    if (a->g_c == 1 ? (a->g_pad < a->C || a->g_pad > a->g_v || (a->g_pad & 3)) : a->g_pad != 0) return OCCD_EINVAL;
    RLP q{};
    fill(q, a);
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("render_depth_bwd_voxels", st, (double)q.total * a->C * 4.0, (double)q.total * (8.0 * a->C + 16.0));
    const dim3 grid(grid_for(q.total));
    if (a->C <= 4) hipLaunchKernelGGL(bwd_voxels_kernel<4>, grid, dim3(256), 0, st, q);
    else if (a->C <= 12) hipLaunchKernelGGL(bwd_voxels_kernel<12>, grid, dim3(256), 0, st, q);
    else if (a->C <= 20) hipLaunchKernelGGL(bwd_voxels_kernel<20>, grid, dim3(256), 0, st, q);
    else hipLaunchKernelGGL(bwd_voxels_kernel<32>, grid, dim3(256), 0, st, q);
    return occd::check_launch();
}
