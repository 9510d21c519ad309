// Voxel-centroid -> pixel projection shared by lift.hip (occd_project_voxels, the fused lift) and targets.hip (frustum
// training targets): one definition, so the tables, the in-kernel lift and the targets see the same integers.
#pragma once
#include <hip/hip_runtime.h>

namespace occd {

// SURVEY.md 8(f) row N2, one voxel: occdepth/data/utils/helpers.py:94-169 with fusion.py:203-217 (vox2world: float32
// origin, float64 arithmetic, float32 store), :518-522 (rigid transform in float64) and :336-337 (round(x * fx / z + cx),
// float32 intrinsics, numpy round-half-even).  Every product / sum is an explicitly rounded IEEE double operation (no FMA
// contraction) so the pixels are the ones numpy computes.  Returns the FOV flag.
__device__ __forceinline__ bool project_one(const double* __restrict__ E, double fx, double fy, double cx, double cy,
                                            double vox_size, const float* origin, int ix, int iy, int iz, int img_w,
                                            int img_h, long& px, long& py, double& camz) {
    const int idx[3] = {ix, iy, iz};
    double pt[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double a = __dadd_rn((double)origin[j], __dmul_rn(vox_size, (double)(float)idx[j]));
        pt[j] = (double)(float)__dadd_rn(a, __dmul_rn(vox_size, 0.5));
    }
    double cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double acc = __dmul_rn(E[r * 4 + 0], pt[0]);
        acc = __dadd_rn(acc, __dmul_rn(E[r * 4 + 1], pt[1]));
        acc = __dadd_rn(acc, __dmul_rn(E[r * 4 + 2], pt[2]));
        cam[r] = __dadd_rn(acc, E[r * 4 + 3]);
    }
    double xr = rint(__dadd_rn(__ddiv_rn(__dmul_rn(cam[0], fx), cam[2]), cx));
    double yr = rint(__dadd_rn(__ddiv_rn(__dmul_rn(cam[1], fy), cam[2]), cy));
    // non-finite projections (z == 0) are clamped like oracle/inputs.py; they are out of the FOV anyway
    xr = isnan(xr) ? -1e9 : fmin(fmax(xr, -1e9), 1e9);
    yr = isnan(yr) ? -1e9 : fmin(fmax(yr, -1e9), 1e9);
    px = (long)xr;
    py = (long)yr;
    camz = cam[2];
    return px >= 0 && px < img_w && py >= 0 && py < img_h && cam[2] > 0.0;
}

}  // namespace occd
