// Shared device-side helpers for the kernels of libocc_hip.so (gfx950 only): ONE definition of everything more than one
// .hip file needs -- vector types, the XCD block remap, the operand splits of the bf16 / fp16 matrix pipe, activations.
// Everything here is __forceinline__: a kernel that calls a helper compiles to what it compiled to with a private copy.
// Per-kernel MFMA macros (shaped by a kernel's register arrays) and one-off types stay in their .hip files.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;   // what ds_read_b64_tr_b16 takes (see tr_frag_bf16x8)

// ------------------------------------------------------------------------------------------------ integer helpers
__device__ __forceinline__ uint32_t occd_fastdiv(uint32_t n, occd::FastDiv f) {
    // branch-free: magic == 0 encodes d == 1
    return __umulhi(n, f.magic) + (f.magic == 0u ? n : 0u);
}

// XCD-aware bijective remap of a linear workgroup id in [0, nwg): the dispatcher deals consecutive workgroups round-robin
// to the 8 XCDs, each with its own L2; the remapped id gives every XCD a contiguous run of ids (the first nwg % 8 XCDs one
// more than the others), so whatever neighbouring tiles share -- halo planes, an operand tile -- meets in one L2.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t bid, uint32_t nwg) {
    const uint32_t q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ------------------------------------------------------------------------------------------------ operand splits
// Names: split<terms>_<format>x<elements>.
//
// Three-term bf16 split: x = hi + mid + lo (round-to-nearest at every step; each term bf16, 8 significant bits: 24
// together), exact for every float32 x whose low parts do not underflow.  With both operands split, six
// v_mfma_f32_32x32x16_bf16 per 16-k step -- (mid,mid), (hi,lo), (lo,hi), (hi,mid), (mid,hi), (hi,hi), smallest first --
// reproduce the float32 product x*w to ~2^-24 relative: float32-level accuracy at 6/16 of the fp32-MFMA time.
__device__ __forceinline__ void split3_bf16x8(f32x4 a, f32x4 b, u32x4& hi, u32x4& mid, u32x4& lo) {
    bf16x8 h = {(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
    float r[8] = {a.x - (float)h[0], a.y - (float)h[1], a.z - (float)h[2], a.w - (float)h[3],
                  b.x - (float)h[4], b.y - (float)h[5], b.z - (float)h[6], b.w - (float)h[7]};
    bf16x8 m, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        m[j] = (__bf16)r[j];
        l[j] = (__bf16)(r[j] - (float)m[j]);
    }
    hi = __builtin_bit_cast(u32x4, h);
    mid = __builtin_bit_cast(u32x4, m);
    lo = __builtin_bit_cast(u32x4, l);
}

__device__ __forceinline__ void split3_bf16x4(f32x4 a, u32x2& hi, u32x2& mid, u32x2& lo) {
    bf16x4 h = {(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w};
    float r[4] = {a.x - (float)h[0], a.y - (float)h[1], a.z - (float)h[2], a.w - (float)h[3]};
    bf16x4 m, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = (__bf16)r[j];
        l[j] = (__bf16)(r[j] - (float)m[j]);
    }
    hi = __builtin_bit_cast(u32x2, h);
    mid = __builtin_bit_cast(u32x2, m);
    lo = __builtin_bit_cast(u32x2, l);
}

// Two-term fp16 split of an activation: x' = 2^kF2XExp x = hi + 2^-11 lo' with hi = fp16(x'), lo' = fp16((x' - hi) 2^11)
// (22 significant bits while |x'| >= 2^-13; |x'| >= 65520 becomes +-Inf).  The pre-scale moves that window to
// 2^-14 <= |x| < 32760.  The weight side (occd_pack_weights_f16x2, csrc/conv3d_bf16.hip) folds 2^-kF2XExp into its
// per-channel epilogue factor, so packer and kernels read this one constant.  Three v_mfma_f32_32x32x16_f16 per 16-k step;
// the full scheme is described above K2s3h in csrc/conv3d_c32p.hip.
constexpr int kF2XExp = 1;
__device__ __forceinline__ void split2_f16x8(f32x4 a, f32x4 b, u32x4& hi, u32x4& lo) {
    const float s = (float)(1 << kF2XExp);
    float x[8] = {a.x * s, a.y * s, a.z * s, a.w * s, b.x * s, b.y * s, b.z * s, b.w * s};
    f16x8 h, l;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        h[j] = (_Float16)x[j];
        l[j] = (_Float16)((x[j] - (float)h[j]) * 2048.f);
    }
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// (the same split of four values: the B panels of the 2-D GEMMs are staged in 4-column chunks)
__device__ __forceinline__ void split2_f16x4(f32x4 a, u32x2& hi, u32x2& lo) {
    const float s = (float)(1 << kF2XExp);
    float x[4] = {a.x * s, a.y * s, a.z * s, a.w * s};
    f16x4 h, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        h[j] = (_Float16)x[j];
        l[j] = (_Float16)((x[j] - (float)h[j]) * 2048.f);
    }
    hi = __builtin_bit_cast(u32x2, h);
    lo = __builtin_bit_cast(u32x2, l);
}

// 8 floats -> 8 bf16 (round-to-nearest-even), 16 bytes
__device__ __forceinline__ u32x4 pack_bf16x8(f32x4 a, f32x4 b) {
    bf16x8 r = {(__bf16)a.x, (__bf16)a.y, (__bf16)a.z, (__bf16)a.w, (__bf16)b.x, (__bf16)b.y, (__bf16)b.z, (__bf16)b.w};
    return __builtin_bit_cast(u32x4, r);
}

// MFMA operand fragment (8 consecutive K values of one row / column) out of a tile that lies K-major in LDS, as two
// ds_read_b64_tr_b16: a 16-lane group reads a 4 x 16 block of 16-bit elements row-wise and every lane receives a column
// (semantics pinned on hardware by tools/probe_bf16.hip).  p0: the lane's address in the first 4 K rows; step_bytes: 4 rows.
__device__ __forceinline__ bf16x8 tr_frag_bf16x8(const unsigned char* p0, int step_bytes) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)p0);
    const bf16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(p0 + step_bytes));
    return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ------------------------------------------------------------------------------------------------ activations
namespace occd {
// swish(v) = v * sigmoid(v) on the hardware exp2 / rcp instructions (1 ulp each): the libm expf + IEEE division pair is
// ~25 VALU instructions per element, which in the epilogue of a short-K pointwise GEMM (64 accumulator values per lane)
// costs as much as its MFMA loop.  Result within ~3 ulp of the exact form.
__device__ __forceinline__ float swish_fast(float v) {
    return v * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
}
}  // namespace occd

// The activation codes of the 2-D network's entry points: 0 none, 1 relu, 2 swish / silu, 3 leaky relu (slope).  The two
// functions differ in the swish body ONLY, and that difference is part of each kernel's numerics:
//   act2d_exact -- v / (1 + expf(-v)) with libm expf and IEEE division, the float32 expression ATen's silu evaluates.  The
//       Winograd 3x3 convolutions (K9 wino_output_kernel, csrc/wino2d.hip; K10 wino3x3_kernel, csrc/wino_conv2d.hip) must use
//       it: they stand in for ATen's conv2d + BatchNorm + activation and reproduce its activation, and their epilogue
//       is a small share of a long MFMA loop, so the ~25 instructions cost nothing measurable.
//   act2d_fast  -- occd::swish_fast, within ~3 ulp of the exact form.  The pointwise GEMMs (K11, csrc/pw_gemm.hip), the fused
//       BatchNorm (K13, csrc/bn.hip) and the NCHW kernels of csrc/nchw2d.hip use it: short-K or memory-bound kernels whose
//       time the exact form would show in.
// Moving a kernel from one to the other changes its results by a few ulp: a numerical change, made on purpose or not at all.
__device__ __forceinline__ float act2d_exact(float v, int act, float slope) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return v / (1.f + expf(-v));
    if (act == 3) return v > 0.f ? v : v * slope;
    return v;
}
__device__ __forceinline__ float act2d_fast(float v, int act, float slope) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return occd::swish_fast(v);
    if (act == 3) return v > 0.f ? v : v * slope;
    return v;
}

// The OCCD_ACT_* codes of the 3-D operands on four consecutive channels: relu, or the expf + IEEE division sigmoid (every
// 3-D kernel applies this one function, so an operand has the same bits whichever kernel stages it); other codes pass.
__device__ __forceinline__ f32x4 act3d_x4(f32x4 v, int act) {
    if (act == OCCD_ACT_RELU) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    } else if (act == OCCD_ACT_SIGMOID) {
        v.x = 1.f / (1.f + expf(-v.x)); v.y = 1.f / (1.f + expf(-v.y));
        v.z = 1.f / (1.f + expf(-v.z)); v.w = 1.f / (1.f + expf(-v.w));
    }
    return v;
}
