// K34: which voxels of a frame the camera could see (occd_frame_visibility).  One camera ray per pixel of one view through
// one frame's label volume; every voxel a ray visits, up to and including the first occupied one, is marked.  One thread
// per pixel, a wave = one 8 x 8 pixel tile, as in render.hip: the rays of a tile walk neighbouring voxels, so the label
// gathers and the marks of a wave fall into few cache lines.  Contract: include/occdepth_amd.h.
//
// The walk is occd_render_voxels': csrc/raycast.h holds its set-up and arithmetic, expression for expression, and the loop
// given there is written out here (the reason is given there), so the first occupied voxel of a pixel is the one that kernel
// reports.
//
// Marks are plain byte stores of the constant 1 into a volume that this entry point's own fill kernel zeroed first (same
// stream; no memset node -- captured memset nodes replay wrongly on this runtime).  Many rays
// cross the same voxels near the camera, so a byte that already reads 1 is not stored again; a stale 0 from another
// CU's cache only costs the store.  Whatever the schedule, a byte ends as 1 iff some ray visited it: no read-modify-write
// atomics, no allocation, no host sync.
#include "common.h"
#include "device.h"
#include "raycast.h"

namespace {

using occd::kBlockW;
using occd::kBlockH;
constexpr int kFillThreads = 256;
constexpr int64_t kMaxVox = (int64_t)1 << 28;

struct VisP {
    const void* labels;
    const float* view;
    uint8_t* visible;
    int32_t* hit;
    int32_t H, W, X, Y, Z;
};

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
#pragma clang fp contract(off)   // no product-plus-sum here today (raycast.h has them): a later one stays unfused
    int u, v;
    occd::tile_pixel(u, v);
    if (u >= p.W || v >= p.H) return;
    const int X = p.X, Y = p.Y, Z = p.Z;
    const occd::Ray ray = occd::pixel_ray(p.view, u, v);
    const occd::Entry entry = occd::walk_enter(ray, X, Y, Z);
    int hit = -1;
    if (entry.alive) {
        // the loop of csrc/raycast.h (step 6 and the step bound are kept here: see there)
        const occd::Start s = occd::walk_start(ray, entry, X, Y, Z);
        int ix = s.ix, iy = s.iy, iz = s.iz;
        float mx = s.mx, my = s.my, mz = s.mz;
        const int steps = X + Y + Z + 3;
        for (int n = 0; n < steps; ++n) {
            const int vox = (ix * Y + iy) * Z + iz;               // 0 <= ix < X, ... holds here, always: vox < X Y Z
            if (p.visible[vox] == 0) p.visible[vox] = 1;
            const int lab = occd::load_label<LB>(p.labels, vox);
            if (lab > 0 && lab < 255) { hit = vox; break; }
            const int ax = (mx <= my && mx <= mz) ? 0 : (my <= mz) ? 1 : 2;
            const float m = ax == 0 ? mx : ax == 1 ? my : mz;
            if (!(m < __builtin_inff())) break;
            if (ax == 0) {
                ix += s.sx;
                if (ix < 0 || ix >= X) break;
                mx = occd::boundary_t(ix, s.sx, ray.ox, entry.ix_);
            } else if (ax == 1) {
                iy += s.sy;
                if (iy < 0 || iy >= Y) break;
                my = occd::boundary_t(iy, s.sy, ray.oy, entry.iy_);
            } else {
                iz += s.sz;
                if (iz < 0 || iz >= Z) break;
                mz = occd::boundary_t(iz, s.sz, ray.oz, entry.iz_);
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
