// Stereo depth targets from the batch's rectified image pair: census transform, semi-global matching over the four
// axis-aligned paths, winner-take-all with uniqueness / left-right / inner checks, sub-pixel fit, depth = f B / disparity.
// Integer arithmetic up to the sub-pixel step, so every stage is pinned bit for bit by tests/test_stereo.py's numpy
// restatement.  Contract: include/occdepth_amd.h.  No atomics, no allocation, no host sync, no inter-workgroup
// dependency inside a launch: capture-safe.
//
//   gray_kernel      normalised float image -> uint8 gray, one thread per pixel
//   census_kernel    9 x 7 census, one thread per pixel, the 32 x 8 tile and its 4 x 3 halo staged in LDS
//   paths_kernel     ONE WAVE PER (line, direction): a lane owns the disparities d = 64 j + lane (j < D / 64); the cost is
//                    the popcount of two census words (no cost volume), the d +- 1 neighbours and the minimum over d come
//                    from cross-lane shuffles; loads of cr[y, x - s d] and stores of L[y][x][d] are contiguous over lanes.
//                    Each direction writes its own byte volume (no read-modify-write, any order of the waves).
//   winner_kernel    one wave per pixel group: S = the four volumes summed (4 disparities per lane, 32-bit loads), argmin,
//                    second minimum, the two neighbours of the winner, sub-pixel candidate, the unique / inner flags
//   right_kernel     dR(y, x') = argmin_d S(y, x' + s d, d): 64 right-image pixels per workgroup, S read in 128-byte runs
//   check_kernel     left-right check, final flags and disparity, one thread per pixel
//   depth_kernel     fB (float64 on the device, from the calibration) / disparity
#include "common.h"

namespace {

constexpr int kCensusW = 9, kCensusH = 7;          // window; 62 neighbours
constexpr int kHaloX = kCensusW / 2, kHaloY = kCensusH / 2;
constexpr int kTileW = 32, kTileH = 8;             // census tile = one 256-thread workgroup
constexpr int kAbsent = 1 << 20;                   // stands for a path term that does not exist (d - 1 < 0, d + 1 >= D)
constexpr int kOutside = 62;                       // cost of a candidate that leaves the right image
constexpr int kWinnerPixels = 8;                   // pixels per wave of winner_kernel

// s = -1 for a frame the loader mirrored (ida[b][0][0][0] < 0), +1 otherwise
__device__ __forceinline__ int direction_of(const float* ida, int ida_views, int b) {
    return (ida != nullptr && ida[(int64_t)b * ida_views * 16] < 0.f) ? -1 : 1;
}

struct GrayP {
    const float* img;      // (planes, 3, HW)
    uint8_t* gray;         // (planes, HW)
    int64_t total;         // planes * HW
    int32_t HW;
    float mean[3], std[3];
};

__global__ __launch_bounds__(256) void gray_kernel(GrayP p) {
#pragma clang fp contract(off)   // x * std + mean rounds twice, as the numpy restatement does
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.total) return;
    const int64_t plane = i / p.HW;
    const int32_t px = (int32_t)(i - plane * p.HW);
    const float* src = p.img + plane * 3 * p.HW + px;
    int u[3];
    for (int c = 0; c < 3; ++c) {
        const float v = (src[(int64_t)c * p.HW] * p.std[c] + p.mean[c]) * 255.f;
        u[c] = (int)fminf(fmaxf(rintf(v), 0.f), 255.f);       // a NaN becomes 0
    }
    p.gray[i] = (uint8_t)((77 * u[0] + 150 * u[1] + 29 * u[2] + 128) >> 8);
}

__global__ __launch_bounds__(kTileW * kTileH) void census_kernel(const uint8_t* gray, unsigned long long* census, int H, int W) {
    __shared__ uint8_t tile[kTileH + 2 * kHaloY][kTileW + 2 * kHaloX];
    const int64_t plane = (int64_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    constexpr int kCols = kTileW + 2 * kHaloX, kRows = kTileH + 2 * kHaloY;
    for (int i = threadIdx.x; i < kCols * kRows; i += kTileW * kTileH) {
        const int ty = i / kCols, tx = i - ty * kCols;
        const int y = min(max(y0 + ty - kHaloY, 0), H - 1), x = min(max(x0 + tx - kHaloX, 0), W - 1);   // replicate
        tile[ty][tx] = gray[plane + (int64_t)y * W + x];
    }
    __syncthreads();
    const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const int c = tile[ly + kHaloY][lx + kHaloX];
    unsigned long long word = 0;
    int k = 0;
#pragma unroll
    for (int dy = 0; dy < kCensusH; ++dy)
#pragma unroll
        for (int dx = 0; dx < kCensusW; ++dx) {
            if (dy == kHaloY && dx == kHaloX) continue;
            word |= (unsigned long long)(tile[ly + dy][lx + dx] < c) << k;
            ++k;
        }
    census[plane + (int64_t)y * W + x] = word;
}

struct SgmP {
    const unsigned long long* census;   // (B, 2, H, W)
    const float* ida;
    uint8_t* paths;                     // (B, 4, H, W, D)
    uint16_t* S;                        // (B, H, W, D)
    uint8_t* right;                     // (B, H, W) dR
    int32_t* d0;
    uint8_t* flags;
    float* disp;
    int32_t H, W, D, p1, p2, uniq, ida_views;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m, 64));
    return v;
}

// One wave per (frame, direction, line).  blockIdx.x: [0, H) rows left to right, [H, 2H) rows right to left,
// [2H, 2H + W) columns downwards, [2H + W, 2H + 2W) columns upwards.
template <int K>
__global__ __launch_bounds__(64) void paths_kernel(SgmP p) {
    const int lane = threadIdx.x;
    const int b = blockIdx.y;
    const int H = p.H, W = p.W, D = p.D;
    int line = blockIdx.x, dir, x, y, dx = 0, dy = 0, n;
    if (line < 2 * H) {
        dir = line >= H;
        y = line - dir * H;
        x = dir ? W - 1 : 0;
        dx = dir ? -1 : 1;
        n = W;
    } else {
        line -= 2 * H;
        dir = 2 + (line >= W);
        x = line - (dir - 2) * W;
        y = dir == 3 ? H - 1 : 0;
        dy = dir == 3 ? -1 : 1;
        n = H;
    }
    const int s = direction_of(p.ida, p.ida_views, b);
    const unsigned long long* cl = p.census + (int64_t)b * 2 * H * W;
    const unsigned long long* cr = cl + (int64_t)H * W;
    uint8_t* vol = p.paths + ((int64_t)b * 4 + dir) * H * W * D;

    // the census words of a step: loaded one step ahead, so the loads do not sit on the recurrence's chain
    unsigned long long c_cur, r_cur[K];
    bool in_cur[K];
    auto fetch = [&](int px, int py, unsigned long long& c, unsigned long long (&r)[K], bool (&in)[K]) {
        const int64_t row = (int64_t)py * W;
        c = cl[row + px];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int xr = px - s * (64 * j + lane);
            in[j] = xr >= 0 && xr < W;                        // the index is in range before its load
            r[j] = in[j] ? cr[row + xr] : 0ull;
        }
    };
    fetch(x, y, c_cur, r_cur, in_cur);

    int L[K];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        unsigned long long c_nxt = 0, r_nxt[K];
        bool in_nxt[K];
#pragma unroll
        for (int j = 0; j < K; ++j) { r_nxt[j] = 0; in_nxt[j] = false; }
        if (i + 1 < n) fetch(x + dx, y + dy, c_nxt, r_nxt, in_nxt);

        int cost[K];
#pragma unroll
        for (int j = 0; j < K; ++j) cost[j] = in_cur[j] ? __popcll(c_cur ^ r_cur[j]) : kOutside;
        if (i == 0) {
#pragma unroll
            for (int j = 0; j < K; ++j) L[j] = cost[j];
        } else {
            int nl[K];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                // d - 1: lane - 1 of the same j, lane 63 of j - 1 for lane 0; d + 1: the mirror image
                const int from_below = lane == 63 ? (j > 0 ? L[j - 1] : kAbsent) : L[j];
                const int from_above = lane == 0 ? (j + 1 < K ? L[j + 1] : kAbsent) : L[j];
                const int lo = __shfl(from_below, (lane + 63) & 63, 64);
                const int hi = __shfl(from_above, (lane + 1) & 63, 64);
                const int best = min(min(L[j], m + p.p2), min(lo, hi) + p.p1);
                nl[j] = cost[j] + best - m;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) L[j] = nl[j];
        }
        int lm = L[0];
#pragma unroll
        for (int j = 1; j < K; ++j) lm = min(lm, L[j]);
        m = wave_min(lm);
        uint8_t* out = vol + ((int64_t)y * W + x) * D + lane;
#pragma unroll
        for (int j = 0; j < K; ++j) out[64 * j] = (uint8_t)L[j];

        c_cur = c_nxt;
#pragma unroll
        for (int j = 0; j < K; ++j) { r_cur[j] = r_nxt[j]; in_cur[j] = in_nxt[j]; }
        x += dx;
        y += dy;
    }
}

// A wave takes kWinnerPixels consecutive pixels of a frame; lane l owns the disparities 4 l .. 4 l + 3 (l < D / 4).
__global__ __launch_bounds__(256) void winner_kernel(SgmP p) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int D = p.D;
    const int64_t HW = (int64_t)p.H * p.W;
    const int64_t first = ((int64_t)blockIdx.x * 4 + wave) * kWinnerPixels;
    const bool owns = 4 * lane < D;
    const uint8_t* vol = p.paths + (int64_t)b * 4 * HW * D;
    for (int i = 0; i < kWinnerPixels; ++i) {
        const int64_t px = first + i;
        if (px >= HW) return;                                  // wave-uniform
        int sv[4] = {kAbsent, kAbsent, kAbsent, kAbsent};
        if (owns) {
            sv[0] = sv[1] = sv[2] = sv[3] = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(vol + ((int64_t)v * HW + px) * D + 4 * lane);
                sv[0] += w & 255; sv[1] += (w >> 8) & 255; sv[2] += (w >> 16) & 255; sv[3] += w >> 24;
            }
            uint2 packed;
            packed.x = (uint32_t)sv[0] | ((uint32_t)sv[1] << 16);
            packed.y = (uint32_t)sv[2] | ((uint32_t)sv[3] << 16);
            *reinterpret_cast<uint2*>(p.S + ((int64_t)b * HW + px) * D + 4 * lane) = packed;
        }
        // key = S * 256 + d: the minimum is the lowest S, the lowest d on ties
        int key = kAbsent << 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) key = min(key, owns ? (sv[k] << 8) | (4 * lane + k) : key);
        key = wave_min(key);
        const int d0 = key & 255, best = key >> 8;
        int s2 = kAbsent, va = 0, vb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int d = 4 * lane + k, dist = d > d0 ? d - d0 : d0 - d;
            if (owns && dist > 1) s2 = min(s2, sv[k]);
            if (owns && d == d0 - 1) va = sv[k];
            if (owns && d == d0 + 1) vb = sv[k];
        }
        s2 = wave_min(s2);
        const bool inner = d0 >= 1 && d0 <= D - 2;
        const int a = __shfl(va, inner ? (d0 - 1) >> 2 : 0, 64), bb = __shfl(vb, inner ? (d0 + 1) >> 2 : 0, 64);
        if (lane == 0) {
            const bool unique = 100 * best <= p.uniq * s2;
            float sub = 0.f;
            if (inner) {
                const int den = 2 * (a + bb - 2 * best);
                if (den > 0) sub = (float)(a - bb) / (float)den;
            }
            const int64_t o = (int64_t)b * HW + px;
            p.d0[o] = d0;
            p.flags[o] = (uint8_t)((unique ? 1 : 0) | (inner ? 4 : 0));
            p.disp[o] = (float)d0 + sub;
        }
    }
}

// dR(y, x') = argmin_d S(y, x' + s d, d) over the d that stay inside the image, lowest d on ties.  A workgroup takes 64
// right-image pixels of a row, lane l of every wave the pixel x' = x0 + l.  The waves share out the left-image columns x
// that can match the tile; for one x the lanes read S[y][x][d] at d = s (x - x'), 64 consecutive disparities = 128
// contiguous bytes (walking the diagonal per thread instead touches another cache line in every lane).  Each lane keeps
// the minimum of its own pixel; the four waves' minima meet in LDS.
__global__ __launch_bounds__(256) void right_kernel(SgmP p) {
    __shared__ int part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y = blockIdx.y, b = blockIdx.z;
    const int s = direction_of(p.ida, p.ida_views, b);
    const int W = p.W, D = p.D;
    const int x0 = blockIdx.x * 64, xp = x0 + lane;
    const uint16_t* row = p.S + ((int64_t)b * p.H + y) * W * D;
    const int x_lo = s > 0 ? x0 : max(0, x0 - (D - 1));
    const int x_hi = min(W - 1, s > 0 ? x0 + 63 + D - 1 : x0 + 63);       // 0 <= x_lo, x_hi <= W - 1
    int key = kAbsent << 8;
    for (int x = x_lo + wave; x <= x_hi; x += 4) {
        const int d = s * (x - xp);
        if (d >= 0 && d < D) key = min(key, ((int)row[(int64_t)x * D + d] << 8) | d);
    }
    part[wave][lane] = key;
    __syncthreads();
    if (wave == 0 && xp < W) {                                             // d = 0 (x = x') is always a candidate
        key = min(min(part[0][lane], part[1][lane]), min(part[2][lane], part[3][lane]));
        p.right[((int64_t)b * p.H + y) * W + xp] = (uint8_t)(key & 255);
    }
}

__global__ __launch_bounds__(256) void check_kernel(SgmP p) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= p.W) return;
    const int s = direction_of(p.ida, p.ida_views, b);
    const int64_t rowo = ((int64_t)b * p.H + y) * p.W;
    const int d0 = p.d0[rowo + x];
    const int xr = x - s * d0;
    bool consistent = false;
    if (xr >= 0 && xr < p.W) {
        const int diff = (int)p.right[rowo + xr] - d0;
        consistent = diff >= -1 && diff <= 1;
    }
    const int f = p.flags[rowo + x] | (consistent ? 2 : 0);
    p.flags[rowo + x] = (uint8_t)f;
    if (f != 7) p.disp[rowo + x] = 0.f;
}

struct DepthP {
    const float* disp;
    const double* cam_k;    // (B, V, 3, 3)
    const double* cam_E;    // (B, V, 4, 4)
    float* depth;
    int32_t HW, views;
};

__global__ __launch_bounds__(256) void depth_kernel(DepthP p) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= p.HW) return;
    const double* k = p.cam_k + (int64_t)b * p.views * 9;
    const double* e0 = p.cam_E + (int64_t)b * p.views * 16;
    const double* e1 = e0 + 16;
    const double tx = e0[3] - e1[3], ty = e0[7] - e1[7], tz = e0[11] - e1[11];
    const float fB = (float)(k[0] * sqrt((tx * tx + ty * ty) + tz * tz));
    const float d = p.disp[(int64_t)b * p.HW + i];
    p.depth[(int64_t)b * p.HW + i] = d > 0.f ? fB / d : 0.f;
}

inline int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

inline bool geometry_ok(int32_t batch, int32_t H, int32_t W) {
    return batch > 0 && batch <= 32767 && H > 0 && H <= 65535 && W > 0 && (int64_t)H * W <= 0x7FFFFFFFLL / 4;
}

inline bool disparities_ok(int32_t D) { return D >= 64 && D <= 256 && D % 64 == 0; }

}  // namespace

extern "C" int64_t occd_stereo_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t max_disp) {
    if (!geometry_ok(batch, H, W) || !disparities_ok(max_disp)) return OCCD_EINVAL;
    const int64_t pixels = (int64_t)batch * H * W;
    return align256(pixels * 4 * max_disp) + align256(pixels);
}

extern "C" int occd_stereo_census(const OccdStereoArgs* a, void* stream) {
    if (!a || !a->gray || !a->census) return OCCD_EINVAL;
    if (!geometry_ok(a->batch, a->H, a->W)) return OCCD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t HW = (int64_t)a->H * a->W, planes = (int64_t)a->batch * 2;
    if (a->img) {
        GrayP g;
        g.img = a->img; g.gray = a->gray; g.total = planes * HW; g.HW = (int32_t)HW;
        for (int c = 0; c < 3; ++c) { g.mean[c] = a->mean[c]; g.std[c] = a->std[c]; }
        occd::ProfScope prof("stereo_gray", s, 0.0, (double)planes * HW * 13.0);
        hipLaunchKernelGGL(gray_kernel, dim3((unsigned)((g.total + 255) / 256)), dim3(256), 0, s, g);
        if (occd::check_launch() != OCCD_OK) return OCCD_ELAUNCH;
    }
    occd::ProfScope prof("stereo_census", s, 0.0, (double)planes * HW * 9.0);
    const dim3 grid((unsigned)((a->W + kTileW - 1) / kTileW), (unsigned)((a->H + kTileH - 1) / kTileH), (unsigned)planes);
    hipLaunchKernelGGL(census_kernel, grid, dim3(kTileW * kTileH), 0, s, (const uint8_t*)a->gray,
                       (unsigned long long*)a->census, a->H, a->W);
    return occd::check_launch();
}

extern "C" int occd_stereo_sgm(const OccdStereoArgs* a, void* stream) {
    if (!a || !a->census || !a->workspace || !a->S || !a->d0 || !a->flags || !a->disp) return OCCD_EINVAL;
    if (!geometry_ok(a->batch, a->H, a->W) || !disparities_ok(a->max_disp)) return OCCD_EINVAL;
    if (a->p1 < 0 || a->p1 > a->p2 || a->p2 > 193 || a->uniqueness < 1 || a->uniqueness > 100) return OCCD_EINVAL;
    if (a->ida && a->ida_views <= 0) return OCCD_EINVAL;
    if (2 * (int64_t)a->H + 2 * (int64_t)a->W > 0x7FFFFFFFLL) return OCCD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t pixels = (int64_t)a->batch * a->H * a->W, HW = (int64_t)a->H * a->W;
    const int D = a->max_disp;
    SgmP p;
    p.census = (const unsigned long long*)a->census;
    p.ida = a->ida;
    p.paths = (uint8_t*)a->workspace;
    p.right = p.paths + align256(pixels * 4 * D);
    p.S = a->S; p.d0 = a->d0; p.flags = a->flags; p.disp = a->disp;
    p.H = a->H; p.W = a->W; p.D = D; p.p1 = a->p1; p.p2 = a->p2; p.uniq = a->uniqueness; p.ida_views = a->ida_views;
    {
        occd::ProfScope prof("stereo_paths", s, 0.0, (double)pixels * (4.0 * D + 4.0 * 16.0));
        const dim3 grid((unsigned)(2 * a->H + 2 * a->W), (unsigned)a->batch);
        switch (D / 64) {
            case 1: hipLaunchKernelGGL(paths_kernel<1>, grid, dim3(64), 0, s, p); break;
            case 2: hipLaunchKernelGGL(paths_kernel<2>, grid, dim3(64), 0, s, p); break;
            case 3: hipLaunchKernelGGL(paths_kernel<3>, grid, dim3(64), 0, s, p); break;
            default: hipLaunchKernelGGL(paths_kernel<4>, grid, dim3(64), 0, s, p); break;
        }
        if (occd::check_launch() != OCCD_OK) return OCCD_ELAUNCH;
    }
    {
        occd::ProfScope prof("stereo_winner", s, 0.0, (double)pixels * (6.0 * D + 9.0));
        const dim3 grid((unsigned)((HW + 4 * kWinnerPixels - 1) / (4 * kWinnerPixels)), (unsigned)a->batch);
        hipLaunchKernelGGL(winner_kernel, grid, dim3(256), 0, s, p);
        if (occd::check_launch() != OCCD_OK) return OCCD_ELAUNCH;
    }
    const dim3 rows((unsigned)((a->W + 255) / 256), (unsigned)a->H, (unsigned)a->batch);
    {
        occd::ProfScope prof("stereo_right", s, 0.0, (double)pixels * (2.0 * D + 1.0));
        const dim3 tiles((unsigned)((a->W + 63) / 64), (unsigned)a->H, (unsigned)a->batch);
        hipLaunchKernelGGL(right_kernel, tiles, dim3(256), 0, s, p);
        if (occd::check_launch() != OCCD_OK) return OCCD_ELAUNCH;
    }
    occd::ProfScope prof("stereo_check", s, 0.0, (double)pixels * 15.0);
    hipLaunchKernelGGL(check_kernel, rows, dim3(256), 0, s, p);
    return occd::check_launch();
}

extern "C" int occd_stereo_depth(const OccdStereoArgs* a, void* stream) {
    if (!a || !a->disp || !a->depth || !a->cam_k || !a->cam_E) return OCCD_EINVAL;
    if (!geometry_ok(a->batch, a->H, a->W) || a->calib_views < 2) return OCCD_EINVAL;
    DepthP p;
    p.disp = a->disp; p.cam_k = a->cam_k; p.cam_E = a->cam_E; p.depth = a->depth;
    p.HW = a->H * a->W; p.views = a->calib_views;
    hipStream_t s = (hipStream_t)stream;
    occd::ProfScope prof("stereo_depth", s, 0.0, (double)a->batch * p.HW * 8.0);
    hipLaunchKernelGGL(depth_kernel, dim3((unsigned)((p.HW + 255) / 256), (unsigned)a->batch), dim3(256), 0, s, p);
    return occd::check_launch();
}
