// Temporal fusion of class probabilities over a sequence (occd_fuse_store, occd_fuse_frames).  Contract:
// include/occdepth_amd.h.
//
// Store pass: softmax of one frame's logits into float32 rows, one row of `pitch` floats per voxel (a ring slot).  A
// workgroup takes 256 consecutive voxels through LDS, so that its reads -- (C, S) planes, or 16-byte pieces of channels-last
// rows -- and its row writes are both contiguous.  Channels-last rows that are not 16-byte aligned go through
// occd_softmax_channels (one thread per row, scalar loads; at 256 x 256 x 32 x 20 it takes 0.91 ms against 0.10 ms).
//
// Fuse pass: a gather.  Every target voxel reads one row per source, each row exactly once per launch, so the kernel lives
// on HBM latency and bandwidth (the lift's regime).  Layout: a group of LPV lanes owns one voxel, lane q of the group holds
// channels [4q, 4q + 4) -- one 16-byte load per source, one float4 accumulator; consecutive groups of a wave are
// consecutive voxels along z, which under the small rotations of driving land in consecutive source rows: a wave's load
// instruction then covers 64 / LPV neighbouring rows, whole 128-byte lines.  The loads of all sources are issued
// unconditionally (clamped address) before any of them is used and masked afterwards, as in lift.hip.  One group, one
// voxel, sources in ascending k: no atomics, and the bytes written do not depend on the schedule.
#include "common.h"
#include "device.h"

namespace {

constexpr int kStoreVox = 256;    // voxels (= threads) per workgroup of the store pass

// ROWS: channels-last rows, `stride` floats apart, read in 16-byte pieces; else planes, `stride` floats apart
template <bool ROWS>
__global__ void __launch_bounds__(kStoreVox) fuse_store_kernel(const float* __restrict__ logits, float* __restrict__ rows,
                                                              long S, int C, long stride, int pitch) {
    __shared__ float tile[32][kStoreVox + 1];      // + 1: the row pieces of one voxel land on different banks
    __shared__ float mx_s[kStoreVox], sum_s[kStoreVox];
    const int tid = threadIdx.x;
    const long v0 = (long)blockIdx.x * kStoreVox;
    const int nv = (int)((S - v0) < kStoreVox ? (S - v0) : kStoreVox);
    if (ROWS) {
        const int nq = (C + 3) >> 2;               // only the pieces that hold classes: the row's pad is never read
        for (int e = tid; e < nv * nq; e += kStoreVox) {
            const int vv = e / nq, c0 = (e - vv * nq) * 4;
            const f32x4 x = *reinterpret_cast<const f32x4*>(logits + (size_t)(v0 + vv) * stride + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c0 + i < C) tile[c0 + i][vv] = x[i];
        }
        __syncthreads();
    }
    if (tid < nv) {
        float mx = -__builtin_inff();
        for (int c = 0; c < C; ++c) {
            float x;
            if (ROWS) {
                x = tile[c][tid];
            } else {
                x = logits[(size_t)c * stride + v0 + tid];
                tile[c][tid] = x;
            }
            mx = fmaxf(mx, x);
        }
        float sum = 0.f;
        for (int c = 0; c < C; ++c) sum += expf(tile[c][tid] - mx);
        mx_s[tid] = mx;
        sum_s[tid] = sum;
    }
    __syncthreads();
    // the workgroup's rows are one contiguous run of nv * pitch floats: 16-byte stores in address order
    const int q4 = pitch >> 2;
    f32x4* out = reinterpret_cast<f32x4*>(rows + (size_t)v0 * pitch);
    for (int e = tid; e < nv * q4; e += kStoreVox) {
        const int vv = e / q4, c0 = (e - vv * q4) * 4;
        const float mx = mx_s[vv], sum = sum_s[vv];
        f32x4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = c0 + i < C ? expf(tile[c0 + i][vv] - mx) / sum : 0.f;
        out[e] = o;
    }
}

struct FuseP {
    OccdFuseArgs a;
    uint32_t n_vox;
};

// LPV lanes per voxel (4: C <= 16, 8: C <= 32); KB: the number of sources rounded up to a power of two -- the slots
// [K, KB) repeat source 0 with `ok` forced off, so the load phase has no condition in it.
template <int LPV, int KB>
__global__ void __launch_bounds__(256) fuse_frames_kernel(const FuseP p) {
    const OccdFuseArgs& a = p.a;
    const int tid = threadIdx.x;
    const int sub = tid % LPV;
    // every XCD takes one contiguous run of workgroups, i.e. one slab of x: rows that straddle a 128-byte line at the seam
    // of two workgroups meet in one L2
    const uint32_t bid = xcd_remap(blockIdx.x, gridDim.x);
    const uint32_t n = (bid * 256u + (uint32_t)tid) / LPV;
    const bool vox_ok = n < p.n_vox;
    const uint32_t nn = vox_ok ? n : p.n_vox - 1;
    const uint32_t ij = nn / (uint32_t)a.Z;
    const int l = (int)(nn - ij * (uint32_t)a.Z);
    const int i = (int)(ij / (uint32_t)a.Y);
    const int j = (int)(ij - (uint32_t)i * (uint32_t)a.Y);
    const float fx = (float)i + 0.5f, fy = (float)j + 0.5f, fz = (float)l + 0.5f;
    const float fX = (float)a.X, fY = (float)a.Y, fZ = (float)a.Z;
    const int c0 = sub * 4;
    const bool ch_ok = c0 < a.C;               // this lane's 16 bytes hold at least one class
    const int cc = ch_ok ? c0 : 0;

    f32x4 row[KB];
    uint8_t mk[KB];
    bool ok[KB];
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const int ks = k < a.K ? k : 0;
        const float* g = a.affine[ks];
        const float sx = fmaf(g[0], fx, fmaf(g[1], fy, fmaf(g[2], fz, g[9])));
        const float sy = fmaf(g[3], fx, fmaf(g[4], fy, fmaf(g[5], fz, g[10])));
        const float sz = fmaf(g[6], fx, fmaf(g[7], fy, fmaf(g[8], fz, g[11])));
        // in range as FLOATS first (a NaN fails every comparison), so the conversions below are always defined and, for a
        // non-negative s, truncation is floor
        const bool in = sx >= 0.f && sx < fX && sy >= 0.f && sy < fY && sz >= 0.f && sz < fZ;
        const int ix = in ? (int)sx : 0, iy = in ? (int)sy : 0, iz = in ? (int)sz : 0;
        const uint32_t src = in ? ((uint32_t)ix * (uint32_t)a.Y + (uint32_t)iy) * (uint32_t)a.Z + (uint32_t)iz : 0u;   // < n_vox
        ok[k] = in && k < a.K;
        row[k] = *reinterpret_cast<const f32x4*>(a.rows[ks] + (size_t)src * a.pitch + cc);
        // no mask: the byte is read from the source's own rows (S * pitch * 4 >= S bytes) and dropped, so that this load,
        // too, stands outside any branch
        const bool has = a.masks[ks] != nullptr;
        const uint8_t* m = has ? a.masks[ks] : reinterpret_cast<const uint8_t*>(a.rows[ks]);
        const uint8_t byte = m[src];
        mk[k] = has ? byte : (uint8_t)1;
    }

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f;
    int nobs = 0;
#pragma unroll
    for (int k = 0; k < KB; ++k) {
        const bool use = ok[k] && mk[k] != 0;
        const float w = a.weights[k < a.K ? k : 0];
        acc.x = use ? fmaf(w, row[k].x, acc.x) : acc.x;
        acc.y = use ? fmaf(w, row[k].y, acc.y) : acc.y;
        acc.z = use ? fmaf(w, row[k].z, acc.z) : acc.z;
        acc.w = use ? fmaf(w, row[k].w, acc.w) : acc.w;
        wsum = use ? wsum + w : wsum;
        nobs += use ? 1 : 0;
    }

    // arg-max of acc over the classes, the lowest class on a tie: first inside the lane, then across the LPV lanes
    float best = -__builtin_inff();
    int arg = 0x7fffffff;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = acc[e];
        if (ch_ok && c0 + e < a.C && (v > best || arg == 0x7fffffff)) { best = v; arg = c0 + e; }
    }
#pragma unroll
    for (int d = 1; d < LPV; d <<= 1) {
        const float ob = __shfl_xor(best, d);
        const int oa = __shfl_xor(arg, d);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    if (!vox_ok) return;
    if (sub == 0) {
        a.labels[n] = (uint8_t)(nobs ? arg : 0);
        a.n_obs[n] = (uint8_t)nobs;
    }
    if (a.prob && ch_ok) {
        const float inv = nobs ? 1.f / wsum : 0.f;
        f32x4 o = {acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv};
        if (!nobs) o = f32x4{0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(a.prob + (size_t)n * a.pitch + c0) = o;
    }
}

template <int LPV>
void launch_fuse(const FuseP& p, int kb, dim3 grid, hipStream_t s) {
    switch (kb) {
        case 1: hipLaunchKernelGGL((fuse_frames_kernel<LPV, 1>), grid, dim3(256), 0, s, p); break;
        case 2: hipLaunchKernelGGL((fuse_frames_kernel<LPV, 2>), grid, dim3(256), 0, s, p); break;
        case 4: hipLaunchKernelGGL((fuse_frames_kernel<LPV, 4>), grid, dim3(256), 0, s, p); break;
        default: hipLaunchKernelGGL((fuse_frames_kernel<LPV, 8>), grid, dim3(256), 0, s, p); break;
    }
}

constexpr int64_t kMaxVox = (int64_t)1 << 28;      // 8 lanes per voxel and 32-bit lane indices

bool pitch_ok(int32_t C, int32_t pitch) { return pitch >= ((C + 3) & ~3) && (pitch & 3) == 0; }

}  // namespace

extern "C" int occd_fuse_store(const float* logits, float* rows, int64_t S, int32_t C, int64_t s_c, int64_t s_v,
                               int32_t pitch, void* stream) {
    if (!logits || !rows || S <= 0 || S > kMaxVox || C < 1 || C > 32) return OCCD_EINVAL;
    if (pitch < C || !pitch_ok(C, pitch) || (reinterpret_cast<uintptr_t>(rows) & 15)) return OCCD_EINVAL;
    const bool cl = s_c == 1 && s_v >= C && s_v <= 0x7fffffff;      // channels-last rows (C == 1: either reading is the same)
    if (cl && ((s_v & 3) || s_v < ((C + 3) & ~3) || (reinterpret_cast<uintptr_t>(logits) & 15)))
        return occd_softmax_channels(logits, rows, S, (int32_t)s_v, 0, pitch, 0, C, ((C + 3) & ~3) - C, stream);
    if (!cl && (s_v != 1 || s_c < S)) return OCCD_EINVAL;
    occd::ProfScope prof("fuse_store", (hipStream_t)stream, 0.0, 4.0 * S * (C + pitch));
    const dim3 grid((unsigned)((S + kStoreVox - 1) / kStoreVox));
    if (cl) hipLaunchKernelGGL(fuse_store_kernel<true>, grid, dim3(kStoreVox), 0, (hipStream_t)stream, logits, rows, (long)S, C, (long)s_v, pitch);
    else hipLaunchKernelGGL(fuse_store_kernel<false>, grid, dim3(kStoreVox), 0, (hipStream_t)stream, logits, rows, (long)S, C, (long)s_c, pitch);
    return occd::check_launch();
}

extern "C" int occd_fuse_frames(const OccdFuseArgs* a, void* stream) {
    if (!a || !a->labels || !a->n_obs) return OCCD_EINVAL;
    if (a->C < 1 || a->C > 32 || a->K < 1 || a->K > OCCD_FUSE_MAX_SOURCES) return OCCD_EINVAL;
    if (a->X <= 0 || a->Y <= 0 || a->Z <= 0 || (int64_t)a->X * a->Y * a->Z > kMaxVox) return OCCD_EINVAL;
    if (a->pitch < a->C || !pitch_ok(a->C, a->pitch) || (reinterpret_cast<uintptr_t>(a->prob) & 15)) return OCCD_EINVAL;
    for (int k = 0; k < a->K; ++k)
        if (!a->rows[k] || (reinterpret_cast<uintptr_t>(a->rows[k]) & 15)) return OCCD_EINVAL;
    FuseP p;
    p.a = *a;
    p.n_vox = (uint32_t)((int64_t)a->X * a->Y * a->Z);
    const int lpv = a->C <= 16 ? 4 : 8;
    const int kb = a->K <= 1 ? 1 : a->K <= 2 ? 2 : a->K <= 4 ? 4 : 8;
    const int64_t lanes = (int64_t)p.n_vox * lpv;
    const dim3 grid((unsigned)((lanes + 255) / 256));
    const double bytes = (double)p.n_vox * (a->K * 4.0 * a->C + 2.0 + (a->prob ? 4.0 * a->C : 0.0));
    occd::ProfScope prof("fuse_frames", (hipStream_t)stream, 0.0, bytes);
    if (lpv == 4) launch_fuse<4>(p, kb, grid, (hipStream_t)stream);
    else launch_fuse<8>(p, kb, grid, (hipStream_t)stream);
    return occd::check_launch();
}
