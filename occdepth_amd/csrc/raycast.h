// The float32 voxel walk of the ray-cast kernels, for K31 map_render.hip, K34 visibility.hip and K35 ray_metric.hip: the
// pixel ray, the finite and slab tests, the clamped first voxel and the boundary times are formed here and nowhere else in
// those three.  Plainly: this set-up exists three times in csrc/ -- here, in K27 render.hip and in K36 render_loss.hip,
// which keep their own text because on this header they measured 1.5 - 1.9 % slower (profiles/raycast_refactor.txt) --
// and the loop over it (step 6 and the step bound, below) five times, once per kernel.  All copies hold the same
// expressions in the same order, so the kernels agree bit for bit; the GPU tests hold them to each other and to the numpy
// restatements (tests/test_render.py cast_ref and its kin), which repeat the arithmetic in this order.  Contract:
// include/occdepth_amd.h (occd_render_voxels).  Every function that multiplies and adds turns fp contraction off: each
// product and sum rounds once.  The numbered steps are the ones the restatements and the contract follow.
#pragma once
#include "common.h"

namespace occd {

constexpr int kTile = 8;                   // a wave's pixel tile is kTile x kTile
constexpr int kBlockW = 16, kBlockH = 16;  // 4 waves = 2 x 2 tiles per workgroup

// The pixel of this thread: a wave is one 8 x 8 tile, so that its rays walk neighbouring voxels and its gathers fall
// into few cache lines.
__device__ __forceinline__ void tile_pixel(int& u, int& v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u = blockIdx.x * kBlockW + (wave & 1) * kTile + (lane & 7);
    v = blockIdx.y * kBlockH + (wave >> 1) * kTile + (lane >> 3);
}

struct Ray {
    float ox, oy, oz, dx, dy, dz;          // origin and direction in grid units (one voxel = 1)
};

// the ray of pixel (u, v) from the 18 floats of an OccdRenderView
__device__ __forceinline__ Ray pixel_ray(const float* g, int u, int v) {
#pragma clang fp contract(off)
    const float fu = (float)u + 0.5f, fv = (float)v + 0.5f;
    Ray r;
    r.ox = g[0] + fu * g[3] + fv * g[6]; r.oy = g[1] + fu * g[4] + fv * g[7]; r.oz = g[2] + fu * g[5] + fv * g[8];
    r.dx = g[9] + fu * g[12] + fv * g[15]; r.dy = g[10] + fu * g[13] + fv * g[16]; r.dz = g[11] + fu * g[14] + fv * g[17];
    return r;
}

struct Entry {
    bool alive;                            // the ray is finite and crosses the box [0,X] x [0,Y] x [0,Z]
    float t, tf;                           // where it enters (0 when the origin lies inside) and where it leaves
    int face;                              // the axis of the slab it enters through, 3 when the origin lies inside
    float ix_, iy_, iz_;                   // 1 / direction, 0 for a zero component
};

__device__ __forceinline__ Entry walk_enter(const Ray& r, int X, int Y, int Z) {
#pragma clang fp contract(off)
    const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz;
    const float inf = __builtin_inff();
    const float fX = (float)X, fY = (float)Y, fZ = (float)Z;
    Entry e;
    e.alive = (ox - ox) + (oy - oy) + (oz - oz) + (dx - dx) + (dy - dy) + (dz - dz) == 0.f;   // all finite
    e.t = 0.f;
    e.face = 3;
    // 1-4: slab test; a zero component is parallel: inside or outside by the origin, never a division
    float tn = -inf, tf = inf;
    int axis = 3;
    const float ix_ = dx != 0.f ? 1.f / dx : 0.f, iy_ = dy != 0.f ? 1.f / dy : 0.f, iz_ = dz != 0.f ? 1.f / dz : 0.f;
    e.ix_ = ix_; e.iy_ = iy_; e.iz_ = iz_;
    if (dx != 0.f) {
        const float a = (0.f - ox) * ix_, c = (fX - ox) * ix_;
        const float n = fminf(a, c);
        if (n > tn) { tn = n; axis = 0; }
        tf = fminf(tf, fmaxf(a, c));
    } else if (!(ox >= 0.f && ox < fX)) e.alive = false;
    if (dy != 0.f) {
        const float a = (0.f - oy) * iy_, c = (fY - oy) * iy_;
        const float n = fminf(a, c);
        if (n > tn) { tn = n; axis = 1; }
        tf = fminf(tf, fmaxf(a, c));
    } else if (!(oy >= 0.f && oy < fY)) e.alive = false;
    if (dz != 0.f) {
        const float a = (0.f - oz) * iz_, c = (fZ - oz) * iz_;
        const float n = fminf(a, c);
        if (n > tn) { tn = n; axis = 2; }
        tf = fminf(tf, fmaxf(a, c));
    } else if (!(oz >= 0.f && oz < fZ)) e.alive = false;
    if (tn > 0.f) { e.t = tn; e.face = axis; }
    if (!(tf >= e.t)) e.alive = false;
    e.tf = tf;
    return e;
}

// t at which the ray leaves voxel index i along an axis it moves on (s = +-1), from the boundary itself (no running sum)
__device__ __forceinline__ float boundary_t(int i, int s, float o, float inv) {
#pragma clang fp contract(off)
    return ((float)(i + (s > 0)) - o) * inv;
}

struct Start {
    int ix, iy, iz;                        // the voxel the ray enters the grid in
    int sx, sy, sz;                        // the sign of each direction component
    float mx, my, mz;                      // boundary_t of that voxel per axis, inf for a zero component
};

// the state a walk starts from; callers copy it into locals of their own
__device__ __forceinline__ Start walk_start(const Ray& r, const Entry& e, int X, int Y, int Z) {
#pragma clang fp contract(off)
    const float ox = r.ox, oy = r.oy, oz = r.oz, dx = r.dx, dy = r.dy, dz = r.dz, t = e.t;
    const float inf = __builtin_inff();
    const float fX = (float)X, fY = (float)Y, fZ = (float)Z;
    Start s;
    // 5: first voxel, clamped as floats so that the conversion is always in range
    s.ix = (int)fminf(fmaxf(floorf(ox + dx * t), 0.f), fX - 1.f);
    s.iy = (int)fminf(fmaxf(floorf(oy + dy * t), 0.f), fY - 1.f);
    s.iz = (int)fminf(fmaxf(floorf(oz + dz * t), 0.f), fZ - 1.f);
    s.sx = dx > 0.f ? 1 : dx < 0.f ? -1 : 0; s.sy = dy > 0.f ? 1 : dy < 0.f ? -1 : 0; s.sz = dz > 0.f ? 1 : dz < 0.f ? -1 : 0;
    s.mx = s.sx ? boundary_t(s.ix, s.sx, ox, e.ix_) : inf;
    s.my = s.sy ? boundary_t(s.iy, s.sy, oy, e.iy_) : inf;
    s.mz = s.sz ? boundary_t(s.iz, s.sz, oz, e.iz_) : inf;
    return s;
}

// The loop over this state is written out in each kernel around its per-voxel work, with
//   6: the nearest boundary next, x before y before z on ties: ax = (mx <= my && mx <= mz) ? 0 : (my <= mz) ? 1 : 2; the
//      walk ends when that boundary's t is not below the limit (inf: a zero direction) or the stepped index leaves the
//      grid; otherwise the axis' boundary time is boundary_t of the new index, and face = ax, t = that time;
//   at most X + Y + Z + 3 steps (every step moves one index one way: at most X + Y + Z - 2 are in range).
// As one function that took the per-voxel work as a lambda, hipcc kept the loop's early exits as separate exec-mask
// regions (5 - 8 % more instructions) and the kernels ran 7 - 34 % slower (profiles/raycast_refactor.txt).

template <int BYTES>
__device__ __forceinline__ int load_label(const void* base, int64_t i) {
    if (BYTES == 1) return static_cast<const uint8_t*>(base)[i];
    return static_cast<const uint16_t*>(base)[i];
}

}  // namespace occd
