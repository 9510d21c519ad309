// Headless voxel renderer (occd_render_voxels): one camera ray per pixel through a label volume, first occupied voxel
// wins.  One launch for B frames x V views x H x W pixels, one thread per pixel, a wave = one 8 x 8 pixel tile (the rays
// of a tile walk neighbouring voxels, so the gathers of a wave fall into few cache lines and the volume -- 2-4 MB at
// config 2 -- is served from L2).  No atomics, no allocation, no host sync: capture-safe.  Contract: include/occdepth_amd.h.
//
// This file and csrc/raycast.h hold the same walk, expression for expression: map_render.hip, visibility.hip and
// ray_metric.hip take it from the header, this kernel keeps its own text because on the header its uint8 instantiation
// measured 1.5 % slower on long walks (profiles/raycast_refactor.txt).  A change to the walk is made in both.
#include "common.h"

namespace {

constexpr int kTile = 8;                 // a wave's pixel tile is kTile x kTile
constexpr int kBlockW = 16, kBlockH = 16;  // 4 waves = 2 x 2 tiles per workgroup

struct RenderP {
    const void* labels;
    const void* target;
    const uint8_t* fov;
    const float* views;
    const uint8_t* palette;
    const uint8_t* background;
    uint8_t* rgb;
    int32_t* hit;
    uint8_t* face;
    float* depth;
    int32_t n_views, H, W, X, Y, Z;
    int32_t n_palette, alpha;
    int32_t view_w[OCCD_RENDER_MAX_VIEWS], view_h[OCCD_RENDER_MAX_VIEWS];
    uint8_t bg[4];
};

template <int BYTES>
__device__ __forceinline__ int load_label(const void* base, int64_t i) {
    if (BYTES == 1) return static_cast<const uint8_t*>(base)[i];
    return static_cast<const uint16_t*>(base)[i];
}

// shade[face] / 256: x faces darkest, z faces (the ground seen from above) and the voxel the camera sits in brightest
__device__ __forceinline__ int shade_of(int face) { return face == 0 ? 160 : face == 1 ? 208 : 256; }

// LB: bytes per prediction label; TB: bytes per target label, 0 = class mode (no target)
template <int LB, int TB>
__global__ __launch_bounds__(kBlockW * kBlockH) void render_kernel(RenderP p) {
#pragma clang fp contract(off)   // every product and sum rounds once: tests/test_render.py restates this arithmetic in numpy
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * kBlockW + (wave & 1) * kTile + (lane & 7);
    const int v = blockIdx.y * kBlockH + (wave >> 1) * kTile + (lane >> 3);
    if (u >= p.W || v >= p.H) return;
    const int bv = blockIdx.z, view = bv % p.n_views, b = bv / p.n_views;
    const int64_t pixel = ((int64_t)bv * p.H + v) * p.W + u;
    const int X = p.X, Y = p.Y, Z = p.Z;

    int hit = -1, face = 3;
    float t = 0.f;
    int colour = 0;                                   // palette row of the hit
    if (u < p.view_w[view] && v < p.view_h[view]) {   // the rest of the canvas is background
        const float* g = p.views + (int64_t)bv * 18;
        const float fu = (float)u + 0.5f, fv = (float)v + 0.5f;
        const float ox = g[0] + fu * g[3] + fv * g[6], oy = g[1] + fu * g[4] + fv * g[7], oz = g[2] + fu * g[5] + fv * g[8];
        const float dx = g[9] + fu * g[12] + fv * g[15], dy = g[10] + fu * g[13] + fv * g[16],
                    dz = g[11] + fu * g[14] + fv * g[17];
        const float inf = __builtin_inff();
        const float fX = (float)X, fY = (float)Y, fZ = (float)Z;
        bool alive = (ox - ox) + (oy - oy) + (oz - oz) + (dx - dx) + (dy - dy) + (dz - dz) == 0.f;   // all finite
        // 1-4: slab test; a zero component is parallel: inside or outside by the origin, never a division
        float tn = -inf, tf = inf;
        int axis = 3;
        const float ix_ = dx != 0.f ? 1.f / dx : 0.f, iy_ = dy != 0.f ? 1.f / dy : 0.f, iz_ = dz != 0.f ? 1.f / dz : 0.f;
        if (dx != 0.f) {
            const float a = (0.f - ox) * ix_, c = (fX - ox) * ix_;
            const float n = fminf(a, c);
            if (n > tn) { tn = n; axis = 0; }
            tf = fminf(tf, fmaxf(a, c));
        } else if (!(ox >= 0.f && ox < fX)) alive = false;
        if (dy != 0.f) {
            const float a = (0.f - oy) * iy_, c = (fY - oy) * iy_;
            const float n = fminf(a, c);
            if (n > tn) { tn = n; axis = 1; }
            tf = fminf(tf, fmaxf(a, c));
        } else if (!(oy >= 0.f && oy < fY)) alive = false;
        if (dz != 0.f) {
            const float a = (0.f - oz) * iz_, c = (fZ - oz) * iz_;
            const float n = fminf(a, c);
            if (n > tn) { tn = n; axis = 2; }
            tf = fminf(tf, fmaxf(a, c));
        } else if (!(oz >= 0.f && oz < fZ)) alive = false;
        if (tn > 0.f) { t = tn; face = axis; }
        if (!(tf >= t)) alive = false;
        if (alive) {
            // 5: first voxel, clamped as floats so that the conversion is always in range
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
                const int vox = (ix * Y + iy) * Z + iz;           // 0 <= ix < X, ... holds here, always
                const int lab = load_label<LB>(p.labels, frame + vox);
                const bool occ = lab > 0 && lab < 255;
                if (TB == 0) {
                    if (occ) { hit = vox; colour = min(lab, p.n_palette - 1); break; }
                } else {
                    const int tg = load_label<(TB ? TB : 1)>(p.target, frame + vox);
                    if (tg != 255 && (occ || tg != 0)) {
                        hit = vox;
                        const int err = p.n_palette - 3;          // rows: wrong class, false positive, false negative
                        colour = !occ ? err + 2 : tg == 0 ? err + 1 : tg != lab ? err : min(lab, err - 1);
                        break;
                    }
                }
                // 6: the nearest boundary, x before y before z on ties
                const int ax = (mx <= my && mx <= mz) ? 0 : (my <= mz) ? 1 : 2;
                const float m = ax == 0 ? mx : ax == 1 ? my : mz;
                if (!(m < inf)) break;                            // nothing left to cross (a zero direction)
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
                face = ax;
                t = m;
            }
        }
    }

    int r, gc, bl;
    const uint8_t* back = p.background ? p.background + pixel * 3 : nullptr;
    if (hit >= 0) {
        const uint8_t* c = p.palette + colour * 3;
        const int s = shade_of(face);
        r = (c[0] * s) >> 8; gc = (c[1] * s) >> 8; bl = (c[2] * s) >> 8;
        if (p.fov && !p.fov[(int64_t)b * X * Y * Z + hit]) { r = r / 3 * 2; gc = gc / 3 * 2; bl = bl / 3 * 2; }
        if (back) {
            const int al = p.alpha, be = 256 - p.alpha;
            r = (al * r + be * back[0]) >> 8; gc = (al * gc + be * back[1]) >> 8; bl = (al * bl + be * back[2]) >> 8;
        }
    } else if (back) {
        r = back[0]; gc = back[1]; bl = back[2];
    } else {
        r = p.bg[0]; gc = p.bg[1]; bl = p.bg[2];
    }
    uint8_t* o = p.rgb + pixel * 3;
    o[0] = (uint8_t)r; o[1] = (uint8_t)gc; o[2] = (uint8_t)bl;
    if (p.hit) p.hit[pixel] = hit;
    if (p.face) p.face[pixel] = (uint8_t)(hit >= 0 ? face : 3);
    if (p.depth) p.depth[pixel] = hit >= 0 ? t : __builtin_inff();
}

}  // namespace

extern "C" int occd_render_voxels(const OccdRenderArgs* a, void* stream) {
    if (!a || !a->labels || !a->views || !a->palette || !a->rgb) return OCCD_EINVAL;
    if (a->batch <= 0 || a->n_views <= 0 || a->n_views > OCCD_RENDER_MAX_VIEWS || a->H <= 0 || a->W <= 0) return OCCD_EINVAL;
    if (a->X <= 0 || a->Y <= 0 || a->Z <= 0 || (int64_t)a->X * a->Y * a->Z > 0x7FFFFFFFLL) return OCCD_EINVAL;
    if (a->label_bytes != 1 && a->label_bytes != 2) return OCCD_EINVAL;
    if (a->target && a->target_bytes != 1 && a->target_bytes != 2) return OCCD_EINVAL;
    if (a->n_palette < (a->target ? 4 : 1) || a->n_palette > 65536 || a->alpha < 0 || a->alpha > 256) return OCCD_EINVAL;
    const int64_t bv = (int64_t)a->batch * a->n_views;
    if (bv > 65535) return OCCD_EINVAL;
    RenderP p;
    p.labels = a->labels; p.target = a->target; p.fov = a->fov;
    p.views = reinterpret_cast<const float*>(a->views);
    p.palette = a->palette; p.background = a->background;
    p.rgb = a->rgb; p.hit = a->hit; p.face = a->face; p.depth = a->depth;
    p.n_views = a->n_views; p.H = a->H; p.W = a->W; p.X = a->X; p.Y = a->Y; p.Z = a->Z;
    p.n_palette = a->n_palette; p.alpha = a->alpha;
    if (!occd::fill_view_sizes(a->view_w, a->view_h, a->n_views, a->W, a->H, p.view_w, p.view_h)) return OCCD_EINVAL;
    for (int i = 0; i < 4; ++i) p.bg[i] = a->bg_colour[i];
    const double pixels = (double)bv * a->H * a->W;
    const double volume = (double)a->batch * a->X * a->Y * a->Z * (a->label_bytes + (a->target ? a->target_bytes : 0));
    const double per_pixel = 3.0 + (a->background ? 3.0 : 0.0) + (a->hit ? 4.0 : 0.0) + (a->face ? 1.0 : 0.0) + (a->depth ? 4.0 : 0.0);
    occd::ProfScope prof("render_voxels", (hipStream_t)stream, 0.0, pixels * per_pixel + volume);
    const dim3 grid((unsigned)((a->W + kBlockW - 1) / kBlockW), (unsigned)((a->H + kBlockH - 1) / kBlockH), (unsigned)bv);
    const dim3 block(kBlockW * kBlockH);
    hipStream_t s = (hipStream_t)stream;
    const int key = a->label_bytes * 4 + (a->target ? a->target_bytes : 0);
    switch (key) {
        case 4: hipLaunchKernelGGL((render_kernel<1, 0>), grid, block, 0, s, p); break;
        case 5: hipLaunchKernelGGL((render_kernel<1, 1>), grid, block, 0, s, p); break;
        case 6: hipLaunchKernelGGL((render_kernel<1, 2>), grid, block, 0, s, p); break;
        case 8: hipLaunchKernelGGL((render_kernel<2, 0>), grid, block, 0, s, p); break;
        case 9: hipLaunchKernelGGL((render_kernel<2, 1>), grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL((render_kernel<2, 2>), grid, block, 0, s, p); break;
    }
    return occd::check_launch();
}
