// K31, occd_map_render: the sequence map (semantic_map.MapVolume) ray-cast to images without densifying it.  Two levels:
// a directory of 16^3-voxel bricks over the map's window and one 4 KB row of labels per brick.  One ray per pixel, one
// thread per pixel, a wave = one 8 x 8 pixel tile, as in render.hip: a tile's rays walk the same few bricks, so its
// label gathers fall into few 4 KB rows and its directory reads into few lines, both served from L2.  Ray set-up and starting
// state are render.hip's, taken from csrc/raycast.h; the loop is this kernel's own.  Inside a present
// brick it steps as the loop of raycast.h does (step 6); an absent brick is left in one step that lands on the very state the
// voxel walk would have reached (contract and proof sketch: include/occdepth_amd.h).  The walk is latency-bound and
// divergent by nature (a lane is idle once its ray has ended); the loop body is kept short and branch-light, the
// directory entry is re-read only when the ray changes brick, and the per-ray state stays in about 50 registers, no scratch.
// Measured (profiles/map_render_ab.txt): the skip pays for rays along a thin window's short axis and loses elsewhere.
// No atomics, no allocation, no host sync: capture-safe.
#include "common.h"
#include "raycast.h"

namespace {

using occd::kBlockW;
using occd::kBlockH;
constexpr int kBrick = OCCD_MAP_BRICK, kBrickVox = kBrick * kBrick * kBrick;
static_assert(kBrick == 16, "the index arithmetic below shifts by 4");

struct MapRenderP {
    const uint8_t* labels;
    const uint8_t* target;
    const int32_t* cells;
    const float* views;
    const uint8_t* palette;
    const uint8_t* background;
    uint8_t* rgb;
    int64_t* hit;
    uint8_t* face;
    float* depth;
    int32_t gx, gy, gz, n_rows, H, W;
    int32_t n_palette, alpha, walk_absent;
    float t_max;
    int32_t view_w[OCCD_RENDER_MAX_VIEWS], view_h[OCCD_RENDER_MAX_VIEWS];
    uint8_t bg[4];
};

__device__ __forceinline__ int shade_of(int face) { return face == 0 ? 160 : face == 1 ? 208 : 256; }

// the brick's last voxel index along an axis the ray moves on
__device__ __forceinline__ int last_of(int i, int s) { return s > 0 ? (i | (kBrick - 1)) : (i & ~(kBrick - 1)); }

// An absent brick is left through axis A at time M.  Axis B's index becomes the first one whose crossing does not
// precede (M, A) in the voxel walk's merge order: m_b <= M when B < A (B wins that tie), m_b < M when B > A.
// One call per axis and no branch on the exit axis: the lanes of a wave leave their bricks through different faces, and
// code per face would run once for each.  `exits`: B is the exit axis itself, which goes one past `last`; `ties`: B < A.
__device__ __forceinline__ int advance_to(int i, int last, int s, float o, float d, float inv, float M, bool exits, bool ties) {
#pragma clang fp contract(off)
    const int up = s > 0;
    const bool moves = s != 0 && !exits;
    const float lo = (float)(up ? i : last), hi = (float)(up ? last : i);
    int e = (int)fminf(fmaxf(floorf(o + d * M), lo), hi);              // the estimate, between i and last
    const auto precedes = [&](int j) {
        const float m = ((float)(j + up) - o) * inv;
        return ties ? m <= M : m < M;
    };
    while (moves && e != i && !precedes(e - s)) e -= s;                // 0.08 single steps per ray on average, both loops
    while (moves && e != last && precedes(e)) e += s;
    return exits ? last + s : moves ? e : i;
}

// ERR: error mode (a target row beside every label row)
template <bool ERR>
__global__ __launch_bounds__(kBlockW * kBlockH) void map_render_kernel(MapRenderP p) {
#pragma clang fp contract(off)   // no product-plus-sum here today (raycast.h has them): a later one stays unfused
    int u, v;
    occd::tile_pixel(u, v);
    if (u >= p.W || v >= p.H) return;
    const int view = blockIdx.z;
    const int64_t pixel = ((int64_t)view * p.H + v) * p.W + u;
    const int X = p.gx * kBrick, Y = p.gy * kBrick, Z = p.gz * kBrick;

    int64_t hit = -1;
    int face = 3;
    float t = 0.f;
    int colour = 0;
    if (u < p.view_w[view] && v < p.view_h[view]) {
        const occd::Ray ray = occd::pixel_ray(p.views + (int64_t)view * 18, u, v);
        const occd::Entry entry = occd::walk_enter(ray, X, Y, Z);
        if (entry.alive) {
            // the state every walk starts from; the two-level loop below is this kernel's own
            const occd::Start st = occd::walk_start(ray, entry, X, Y, Z);
            const float ox = ray.ox, oy = ray.oy, oz = ray.oz, dx = ray.dx, dy = ray.dy, dz = ray.dz;
            const float inf = __builtin_inff();
            const float ix_ = entry.ix_, iy_ = entry.iy_, iz_ = entry.iz_;
            const int sx = st.sx, sy = st.sy, sz = st.sz;
            int ix = st.ix, iy = st.iy, iz = st.iz;
            float mx = st.mx, my = st.my, mz = st.mz;
            t = entry.t;
            face = entry.face;
            const auto bound_x = [&](int i) { return occd::boundary_t(i, sx, ox, ix_); };
            const auto bound_y = [&](int i) { return occd::boundary_t(i, sy, oy, iy_); };
            const auto bound_z = [&](int i) { return occd::boundary_t(i, sz, oz, iz_); };
            const float t_max = p.t_max;
            const int steps = kBrick * (p.gx + p.gy + p.gz) + 3;
            int cell_at = -1, row = -1;                       // the directory entry of the brick the ray is in
            for (int n = 0; n < steps; ++n) {
                // 0 <= ix < X, ... holds here, always
                const int cell = ((ix >> 4) * p.gy + (iy >> 4)) * p.gz + (iz >> 4);
                if (cell != cell_at) {
                    cell_at = cell;
                    row = p.cells[cell];
                    if (row >= p.n_rows) row = -1;            // no row to read: absent
                }
                if (row >= 0) {
                    const int local = (((ix & 15) << 4) + (iy & 15)) * kBrick + (iz & 15);
                    const int64_t at = (int64_t)row * kBrickVox + local;
                    const int lab = p.labels[at];
                    const bool occ = lab > 0 && lab < 255;
                    bool vis = occ;
                    int tg = 0;
                    if (ERR) {
                        tg = p.target[at];
                        vis = tg != 255 && (occ || tg != 0);
                    }
                    if (vis) {
                        if (t <= t_max) {                     // a hit past t_max is a miss, and the walk ends there too
                            hit = at;
                            const int err = p.n_palette - 3;  // rows: wrong class, false positive, false negative
                            colour = !ERR ? min(lab, p.n_palette - 1)
                                          : !occ ? err + 2 : tg == 0 ? err + 1 : tg != lab ? err : min(lab, err - 1);
                        }
                        break;
                    }
                }
                if (row >= 0 || p.walk_absent) {
                    // one voxel on: the nearest boundary, x before y before z on ties (raycast.h step 6)
                    const int ax = (mx <= my && mx <= mz) ? 0 : (my <= mz) ? 1 : 2;
                    const float m = ax == 0 ? mx : ax == 1 ? my : mz;
                    if (!(m < inf) || m > t_max) break;       // nothing left to cross, or every later voxel is past t_max
                    if (ax == 0) {
                        ix += sx;
                        if (ix < 0 || ix >= X) break;
                        mx = bound_x(ix);
                    } else if (ax == 1) {
                        iy += sy;
                        if (iy < 0 || iy >= Y) break;
                        my = bound_y(iy);
                    } else {
                        iz += sz;
                        if (iz < 0 || iz >= Z) break;
                        mz = bound_z(iz);
                    }
                    face = ax;
                    t = m;
                } else {
                    // an absent brick, left in one step through the first of its boundaries in merge order
                    const int lx = last_of(ix, sx), ly = last_of(iy, sy), lz = last_of(iz, sz);
                    const float Mx = sx ? bound_x(lx) : inf, My = sy ? bound_y(ly) : inf, Mz = sz ? bound_z(lz) : inf;
                    const int ax = (Mx <= My && Mx <= Mz) ? 0 : (My <= Mz) ? 1 : 2;
                    const float M = ax == 0 ? Mx : ax == 1 ? My : Mz;
                    if (!(M < inf) || M > t_max) break;
                    ix = advance_to(ix, lx, sx, ox, dx, ix_, M, ax == 0, true);        // x wins every tie it is in
                    iy = advance_to(iy, ly, sy, oy, dy, iy_, M, ax == 1, ax == 2);
                    iz = advance_to(iz, lz, sz, oz, dz, iz_, M, ax == 2, false);
                    if ((unsigned)ix >= (unsigned)X || (unsigned)iy >= (unsigned)Y || (unsigned)iz >= (unsigned)Z) break;
                    mx = sx ? bound_x(ix) : inf;
                    my = sy ? bound_y(iy) : inf;
                    mz = sz ? bound_z(iz) : inf;
                    face = ax;
                    t = M;
                }
            }
        }
    }

    int r, gc, bl;
    const uint8_t* back = p.background ? p.background + pixel * 3 : nullptr;
    if (hit >= 0) {
        const uint8_t* c = p.palette + colour * 3;
        const int s = shade_of(face);
        r = (c[0] * s) >> 8; gc = (c[1] * s) >> 8; bl = (c[2] * s) >> 8;
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

extern "C" int occd_map_render(const OccdMapRenderArgs* a, void* stream) {
    if (!a || !a->labels || !a->cells || !a->views || !a->palette || !a->rgb) return OCCD_EINVAL;
    if (a->gx <= 0 || a->gy <= 0 || a->gz <= 0 || a->gx > 65536 || a->gy > 65536 || a->gz > 65536) return OCCD_EINVAL;
    const int64_t n_cells = (int64_t)a->gx * a->gy * a->gz;
    if (n_cells > (1LL << 27) || a->n_rows <= 0) return OCCD_EINVAL;
    if (a->n_views <= 0 || a->n_views > OCCD_RENDER_MAX_VIEWS || a->H <= 0 || a->W <= 0) return OCCD_EINVAL;
    if (a->n_palette < (a->target ? 4 : 1) || a->n_palette > 65536 || a->alpha < 0 || a->alpha > 256) return OCCD_EINVAL;
    if (!(a->t_max >= 0.f) || (a->flags & ~1)) return OCCD_EINVAL;
    MapRenderP p;
    p.labels = a->labels; p.target = a->target; p.cells = a->cells;
    p.views = reinterpret_cast<const float*>(a->views);
    p.palette = a->palette; p.background = a->background;
    p.rgb = a->rgb; p.hit = a->hit; p.face = a->face; p.depth = a->depth;
    p.gx = a->gx; p.gy = a->gy; p.gz = a->gz; p.n_rows = a->n_rows; p.H = a->H; p.W = a->W;
    p.n_palette = a->n_palette; p.alpha = a->alpha; p.walk_absent = a->flags & 1;
    p.t_max = a->t_max;
    if (!occd::fill_view_sizes(a->view_w, a->view_h, a->n_views, a->W, a->H, p.view_w, p.view_h)) return OCCD_EINVAL;
    for (int i = 0; i < 4; ++i) p.bg[i] = a->bg_colour[i];
    const double pixels = (double)a->n_views * a->H * a->W;
    const double map_bytes = (double)a->n_rows * kBrickVox * (a->target ? 2.0 : 1.0) + (double)n_cells * 4.0;
    const double per_pixel = 3.0 + (a->background ? 3.0 : 0.0) + (a->hit ? 8.0 : 0.0) + (a->face ? 1.0 : 0.0) + (a->depth ? 4.0 : 0.0);
    occd::ProfScope prof("map_render", (hipStream_t)stream, 0.0, pixels * per_pixel + map_bytes);
    const dim3 grid((unsigned)((a->W + kBlockW - 1) / kBlockW), (unsigned)((a->H + kBlockH - 1) / kBlockH), (unsigned)a->n_views);
    const dim3 block(kBlockW * kBlockH);
    hipStream_t s = (hipStream_t)stream;
    if (a->target) hipLaunchKernelGGL((map_render_kernel<true>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((map_render_kernel<false>), grid, block, 0, s, p);
    return occd::check_launch();
}
