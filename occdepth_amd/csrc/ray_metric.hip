// K35: score a prediction along sensor rays (occd_ray_metric), the counters of RayIoU ("Fully Sparse 3D Occupancy
// Prediction", Liu et al., 2024).  One thread per (frame b, origin k, ray r): the ray origins[b, k] + t dirs[r] walks the
// grid ONCE and looks at the prediction and at the target in every voxel it visits, each until that volume has its first
// hit; the per-ray outcome (classes and the two entry depths) goes into u32 counters in LDS and from there, one integer
// atomic per non-zero counter and workgroup, into an int64 table (the pattern of the confusion kernel in loss.hip: sums
// of integers, so the result does not depend on the schedule).  64 consecutive rays are a wave; the host orders dirs so
// that they are neighbours (ray_metric.lidar_directions) and their gathers fall into few cache lines.  No allocation, no
// host sync, no memset node: capture-safe.  Contract: include/occdepth_amd.h.
//
// The walk is occd_render_voxels': csrc/raycast.h holds its set-up and arithmetic, expression for expression, and the loop
// given there is written out here (the reason is given there), so the hit of a ray in either volume, and the t it is
// entered at, are what that kernel reports for the same ray.  The voxel sequence depends on the ray alone, so one
// walk that tests two volumes equals two walks.
#include "common.h"
#include "raycast.h"

namespace {

constexpr int kThreads = 256;              // 4 waves of 64 consecutive rays
constexpr int kMaxCounters = 4 + 2 * OCCD_RAY_MAX_CLASSES + OCCD_RAY_MAX_THRESHOLDS * OCCD_RAY_MAX_CLASSES + OCCD_RAY_MAX_THRESHOLDS;

struct RayP {
    const void* pred;
    const void* target;
    const float* origins;
    const float* dirs;
    unsigned long long* counts;
    int32_t n_rays, blocks_per_origin, n_origins;
    int32_t X, Y, Z;
    int32_t C, T, unknown_mode;
    float thr[OCCD_RAY_MAX_THRESHOLDS];
};

using occd::load_label;

// LB: bytes per prediction label; TB: bytes per target label
template <int LB, int TB>
__global__ __launch_bounds__(kThreads) void ray_metric_kernel(RayP p) {
#pragma clang fp contract(off)   // no product-plus-sum here today (raycast.h has them): a later one stays unfused
    __shared__ unsigned int lds[kMaxCounters];
    const int C = p.C, T = p.T;
    const int n_counters = 4 + 2 * C + T * C + T;
    for (int i = threadIdx.x; i < n_counters; i += kThreads) lds[i] = 0u;
    __syncthreads();
    const int bk = blockIdx.x / p.blocks_per_origin;                    // frame b, origin k: bk = b K + k
    const int first = (blockIdx.x - bk * p.blocks_per_origin) * kThreads;
    const int r = first + threadIdx.x;
    if (r < p.n_rays) {
        const int X = p.X, Y = p.Y, Z = p.Z;
        const float* og = p.origins + (int64_t)bk * 3;
        const float* dg = p.dirs + (int64_t)r * 3;
        const occd::Ray ray = {og[0], og[1], og[2], dg[0], dg[1], dg[2]};
        const occd::Entry entry = occd::walk_enter(ray, X, Y, Z);
        int cls_p = 0, cls_g = 0;                  // 0 = no hit; a hit has 0 < class < 255
        float t_p = 0.f, t_g = 0.f;
        bool unknown = false;
        if (entry.alive) {
            const int64_t frame = (int64_t)(bk / p.n_origins) * X * Y * Z;
            const bool drop = p.unknown_mode == 0;
            bool done_p = false, done_g = false;
            // the loop of csrc/raycast.h (step 6 and the step bound are kept here: see there)
            const occd::Start s = occd::walk_start(ray, entry, X, Y, Z);
            int ix = s.ix, iy = s.iy, iz = s.iz;
            float mx = s.mx, my = s.my, mz = s.mz;
            float t = entry.t;
            const int steps = X + Y + Z + 3;
            for (int n = 0; n < steps; ++n) {
                const int vox = (ix * Y + iy) * Z + iz;               // 0 <= ix < X, ... holds here, always: vox < X Y Z
                if (!done_p) {
                    const int lab = load_label<LB>(p.pred, frame + vox);
                    if (lab > 0 && lab < 255) { cls_p = lab; t_p = t; done_p = true; }
                }
                if (!done_g) {
                    const int lab = load_label<TB>(p.target, frame + vox);
                    if (lab > 0 && lab < 255) { cls_g = lab; t_g = t; done_g = true; }
                    else if (drop && lab == 255) { unknown = true; break; }    // nobody knows what is there: the ray is dropped
                }
                if (done_p && done_g) break;
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
                t = m;
            }
        }
        // the outcome of this ray; every index below is < n_counters: classes >= C reach no per-class counter
        unsigned int* gt = lds + 4;
        unsigned int* pr = gt + C;
        unsigned int* tp = pr + C;
        unsigned int* geo = tp + T * C;
        if (unknown) {
            atomicAdd(&lds[2], 1u);
        } else if (cls_g > 0 && cls_g < C) {
            atomicAdd(&lds[1], 1u);
            atomicAdd(&gt[cls_g], 1u);
            if (cls_p == 0) {
                atomicAdd(&lds[3], 1u);
            } else {
                if (cls_p < C) atomicAdd(&pr[cls_p], 1u);
                const float diff = fabsf(t_p - t_g);
                for (int k = 0; k < T; ++k) {
                    if (diff < p.thr[k]) {
                        atomicAdd(&geo[k], 1u);
                        if (cls_p == cls_g) atomicAdd(&tp[k * C + cls_g], 1u);
                    }
                }
            }
        }
    }
    if (threadIdx.x == 0) lds[0] = (unsigned int)min(kThreads, p.n_rays - first);      // first < n_rays for every workgroup
    __syncthreads();
    for (int i = threadIdx.x; i < n_counters; i += kThreads)
        if (lds[i]) atomicAdd(&p.counts[i], (unsigned long long)lds[i]);
}

}  // namespace

extern "C" int occd_ray_metric(const OccdRayMetricArgs* a, void* stream) {
    if (!a || !a->pred || !a->target || !a->origins || !a->dirs || !a->counts) return OCCD_EINVAL;
    if (a->batch <= 0 || a->n_origins <= 0 || a->n_rays <= 0 || a->X <= 0 || a->Y <= 0 || a->Z <= 0) return OCCD_EINVAL;
    if (a->pred_bytes != 1 && a->pred_bytes != 2) return OCCD_EINVAL;
    if (a->target_bytes != 1 && a->target_bytes != 2) return OCCD_EINVAL;
    if (a->n_thresholds <= 0 || a->n_thresholds > OCCD_RAY_MAX_THRESHOLDS) return OCCD_EINVAL;
    if (a->n_classes <= 0 || a->n_classes > OCCD_RAY_MAX_CLASSES) return OCCD_EINVAL;
    if (a->unknown_mode != OCCD_RAY_UNKNOWN_DROP && a->unknown_mode != OCCD_RAY_UNKNOWN_PASS) return OCCD_EINVAL;
    const int64_t S = (int64_t)a->X * a->Y;                     // X Y < 2^62: checked before the third factor
    if (S >= ((int64_t)1 << 31) || S * a->Z >= ((int64_t)1 << 31)) return OCCD_EINVAL;
    const int64_t bk = (int64_t)a->batch * a->n_origins;
    if (bk >= ((int64_t)1 << 31) || bk * a->n_rays >= ((int64_t)1 << 31)) return OCCD_EINVAL;
    RayP p;
    p.pred = a->pred; p.target = a->target; p.origins = a->origins; p.dirs = a->dirs;
    p.counts = reinterpret_cast<unsigned long long*>(a->counts);
    p.n_rays = a->n_rays; p.n_origins = a->n_origins;
    p.blocks_per_origin = (a->n_rays + kThreads - 1) / kThreads;
    p.X = a->X; p.Y = a->Y; p.Z = a->Z;
    p.C = a->n_classes; p.T = a->n_thresholds; p.unknown_mode = a->unknown_mode;
    for (int i = 0; i < OCCD_RAY_MAX_THRESHOLDS; ++i) p.thr[i] = i < a->n_thresholds ? a->thresholds[i] : 0.f;
    hipStream_t s = (hipStream_t)stream;
    // the least traffic: both volumes once (the rays re-read them from the caches), the origins and the directions
    const double bytes = (double)a->batch * (S * a->Z) * (a->pred_bytes + a->target_bytes) + 12.0 * bk + 12.0 * a->n_rays;
    occd::ProfScope prof("ray_metric", s, 0.0, bytes);
    const dim3 grid((unsigned)(bk * p.blocks_per_origin));       // <= B K N < 2^31
    const dim3 block(kThreads);
    switch (a->pred_bytes * 2 + a->target_bytes) {
        case 3: hipLaunchKernelGGL((ray_metric_kernel<1, 1>), grid, block, 0, s, p); break;
        case 4: hipLaunchKernelGGL((ray_metric_kernel<1, 2>), grid, block, 0, s, p); break;
        case 5: hipLaunchKernelGGL((ray_metric_kernel<2, 1>), grid, block, 0, s, p); break;
        default: hipLaunchKernelGGL((ray_metric_kernel<2, 2>), grid, block, 0, s, p); break;
    }
    return occd::check_launch();
}
