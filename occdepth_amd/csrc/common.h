// Shared host-side helpers for libocc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/occdepth_amd.h"

namespace occd {

// Launch-time profiling (HIP events on the launch stream); see prof.cpp.
struct ProfScope {
    ProfScope(const char* kind, hipStream_t s, double flops, double bytes);
    ~ProfScope();
    int slot;
    hipStream_t stream;
};

// conv3d_c32p.hip: persistent weights-stationary kernel for the full-resolution head convolutions.
// 1 = launched, 0 = geometry does not qualify (use the generic kernel), <0 = error.
int try_conv3d_c32_persist(const occd_conv3d_args* a, hipStream_t stream);
// K2s3: the same launches with the 3-way bf16 split (weights = the image of occd_pack_weights_bf16x3); same return convention.
int try_conv3d_c32_slide_x3(const occd_conv3d_args* a, hipStream_t stream, bool f16x2 = false);

// occd_pack_weights*_gather: where element (co, ci, tap) of a packed operator lives in a dense source tensor
constexpr int kMaxTaps = 27;
struct TapMap {
    int64_t s_co, s_ci;
    int32_t ofs[kMaxTaps];
};

// hipFuncAttributeMaxDynamicSharedMemorySize (> 64 KB of LDS) belongs to the (kernel, DEVICE) pair: set once per pair,
// whatever device the calling thread has current (prof.cpp).  Returns OCCD_OK / OCCD_ELAUNCH.
int ensure_big_lds(const void* kernel);

// A/B switches are read BY VALUE, all the same way: unset -> `dflt`; "0" / "" / "off" / "false" -> false; anything
// else -> true.  (`OCCD_PHASE_FAST=0` used to ENABLE the switch because only presence was tested.)
inline bool env_flag(const char* name, bool dflt) {
    const char* e = getenv(name);
    if (e == nullptr) return dflt;
    return !(e[0] == '\0' || e[0] == '0' || e[0] == 'f' || e[0] == 'F' || ((e[0] == 'o' || e[0] == 'O') && (e[1] == 'f' || e[1] == 'F')));
}

inline int check_launch() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? OCCD_OK : OCCD_ELAUNCH;
}

// The view rectangles of a render canvas (occd_render_voxels, occd_map_render), 0 = the whole canvas; false when one is
// larger than the canvas.
inline bool fill_view_sizes(const int32_t* in_w, const int32_t* in_h, int n_views, int W, int H, int32_t* view_w, int32_t* view_h) {
    for (int i = 0; i < OCCD_RENDER_MAX_VIEWS; ++i) {
        const bool used = i < n_views;
        if (used && (in_w[i] < 0 || in_w[i] > W || in_h[i] < 0 || in_h[i] > H)) return false;
        view_w[i] = used ? (in_w[i] ? in_w[i] : W) : 0;
        view_h[i] = used ? (in_h[i] ? in_h[i] : H) : 0;
    }
    return true;
}

// q = n / d for n*d < 2^32 via one mul-hi; d == 1 is encoded as magic 0.  The host fills it, occd_fastdiv (device.h) divides.
struct FastDiv {
    uint32_t magic;
    uint32_t d;
};
inline FastDiv make_fastdiv(uint32_t d) {
    FastDiv f;
    f.d = d;
    f.magic = d <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
    return f;
}

}  // namespace occd
