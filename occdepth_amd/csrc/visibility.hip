// K34: which voxels of a frame the camera could see (occd_frame_visibility).  One camera ray per pixel of one view through
// one frame's label volume; every voxel a ray visits, up to and including the first occupied one, is marked.  One thread
// per pixel, a wave = one 8 x 8 pixel tile, as in render.hip: the rays of a tile walk neighbouring voxels, so the label
// gathers and the marks of a wave fall into few cache lines.  Contract: include/occdepth_amd.h.
//
// The walk is occd_render_voxels' (csrc/render.hip) restated: the same float32 expressions in the same order, so that the
// first occupied voxel of a pixel is the one that kernel reports.  It is restated rather than shared through a header, so
// the sources and code objects of render.hip and map_render.hip stay what they were (that walk is interleaved with the
// face, depth and colour bookkeeping this kernel has no use for; conv3d_tile.h is the precedent for the choice).
//
// Marks are plain byte stores of the constant 1 into a volume that this entry point's own fill kernel zeroed first (same
// stream; no memset node -- captured memset nodes replay wrongly on this runtime).  Many rays
// cross the same voxels near the camera, so a byte that already reads 1 is not stored again; a stale 0 from another
// CU's cache only costs the store.  Whatever the schedule, a byte ends as 1 iff some ray visited it: no read-modify-write
// atomics, no allocation, no host sync.
#include "common.h"
#include "device.h"

namespace {

constexpr int kTile = 8;                   // a wave's pixel tile is kTile x kTile
constexpr int kBlockW = 16, kBlockH = 16;  // 4 waves = 2 x 2 tiles per workgroup
constexpr int kFillThreads = 256;
constexpr int64_t kMaxVox = (int64_t)1 << 28;

struct VisP {
    const void* labels;
    const float* view;
    uint8_t* visible;
    int32_t* hit;
    int32_t H, W, X, Y, Z;
};

template <int BYTES>
__device__ __forceinline__ int load_label(const void* base, int i) {
    if (BYTES == 1) return static_cast<const uint8_t*>(base)[i];
    return static_cast<const uint16_t*>(base)[i];
}

// zeroes out[0, n): 16-byte pieces from the first 16-byte boundary on, the bytes before and after it by thread 0
__global__ __launch_bounds__(kFillThreads) void zero_bytes_kernel(uint8_t* out, int64_t n, int64_t head, int64_t pieces) {
    const int64_t i = (int64_t)blockIdx.x * kFillThreads + threadIdx.x;
    if (i < pieces) {
        u32x4 z;
        z.x = z.y = z.z = z.w = 0u;
        *reinterpret_cast<u32x4*>(out + head + i * 16) = z;
    }
    if (i == 0) {
        for (int64_t k = 0; k < head; ++k) out[k] = 0;
        for (int64_t k = head + pieces * 16; k < n; ++k) out[k] = 0;
    }
}

template <int LB>
__global__ __launch_bounds__(kBlockW * kBlockH) void visibility_kernel(VisP p) {
#pragma clang fp contract(off)   // every product and sum rounds once: tests/test_visibility.py restates this arithmetic in numpy
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * kBlockW + (wave & 1) * kTile + (lane & 7);
    const int v = blockIdx.y * kBlockH + (wave >> 1) * kTile + (lane >> 3);
    if (u >= p.W || v >= p.H) return;
    const int X = p.X, Y = p.Y, Z = p.Z;
    const float* g = p.view;
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
    int hit = -1;
    if (alive) {
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
        const int steps = X + Y + Z + 3;              // every step moves one index one way: at most X + Y + Z - 2 in range
        for (int n = 0; n < steps; ++n) {
            const int vox = (ix * Y + iy) * Z + iz;               // 0 <= ix < X, ... holds here, always: vox < X Y Z
            if (p.visible[vox] == 0) p.visible[vox] = 1;
            const int lab = load_label<LB>(p.labels, vox);
            if (lab > 0 && lab < 255) { hit = vox; break; }
            // the nearest boundary, x before y before z on ties
            const int ax = (mx <= my && mx <= mz) ? 0 : (my <= mz) ? 1 : 2;
            const float m = ax == 0 ? mx : ax == 1 ? my : mz;
            if (!(m < inf)) break;                                // nothing left to cross (a zero direction)
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
        }
    }
    if (p.hit) p.hit[(int64_t)v * p.W + u] = hit;
}

}  // namespace

extern "C" int occd_frame_visibility(const OccdVisibilityArgs* a, void* stream) {
    if (!a || !a->labels || !a->view || !a->visible) return OCCD_EINVAL;
    if (a->H <= 0 || a->W <= 0 || a->X <= 0 || a->Y <= 0 || a->Z <= 0) return OCCD_EINVAL;
    if ((int64_t)a->X * a->Y * a->Z > kMaxVox) return OCCD_EINVAL;
    if (a->label_bytes != 1 && a->label_bytes != 2) return OCCD_EINVAL;
    VisP p;
    p.labels = a->labels; p.view = reinterpret_cast<const float*>(a->view);
    p.visible = a->visible; p.hit = a->hit;
    p.H = a->H; p.W = a->W; p.X = a->X; p.Y = a->Y; p.Z = a->Z;
    hipStream_t s = (hipStream_t)stream;
    const int64_t S = (int64_t)a->X * a->Y * a->Z;
    const double pixels = (double)a->H * a->W;
    // the volume is zeroed, read once and marked; the rays re-read it from the caches
    occd::ProfScope prof("frame_visibility", s, 0.0, S * (2.0 + a->label_bytes) + pixels * (a->hit ? 4.0 : 0.0));
    int64_t head = (int64_t)((16 - (reinterpret_cast<uintptr_t>(a->visible) & 15)) & 15);
    if (head > S) head = S;
    const int64_t pieces = (S - head) / 16;
    const int64_t fill_threads = pieces > 0 ? pieces : 1;
    hipLaunchKernelGGL(zero_bytes_kernel, dim3((unsigned)((fill_threads + kFillThreads - 1) / kFillThreads)), dim3(kFillThreads), 0, s,
                       a->visible, S, head, pieces);
    const dim3 grid((unsigned)((a->W + kBlockW - 1) / kBlockW), (unsigned)((a->H + kBlockH - 1) / kBlockH));
    if (a->label_bytes == 1) hipLaunchKernelGGL(visibility_kernel<1>, grid, dim3(kBlockW * kBlockH), 0, s, p);
    else hipLaunchKernelGGL(visibility_kernel<2>, grid, dim3(kBlockW * kBlockH), 0, s, p);
    return occd::check_launch();
}
