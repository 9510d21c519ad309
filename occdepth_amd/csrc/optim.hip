// Global gradient-norm clipping fused with the AdamW update (include/occdepth_amd.h, "Global gradient-norm clipping"):
//
//   grad_sumsq_kernel    one workgroup per chunk descriptor: sum of squares of <= 8192 gradient elements -> partials[chunk]
//   norm_finalise_kernel one workgroup: partials added in a fixed order -> total_norm, clip_coef (device scalars)
//   clip_adamw_kernel    one workgroup per chunk descriptor: p, m, v updated from clip_coef * g
//   accum_kernel         one workgroup per chunk descriptor: acc = [acc +] scale * g for a window of micro-batches; the one that
//                        closes the window also leaves the chunk's sum of squares of acc in partials[chunk] and advances `step`
//                        (occd_accum_clip_adamw: the norm and update kernels then work on acc and leave at once otherwise)
//
// Reference: Trainer(gradient_clip_val=35) of occdepth/scripts/train.py:188,204 = torch.nn.utils.clip_grad_norm_ between
// the backward and torch.optim.AdamW.step() (occdepth/models/OccDepth.py:582-600 builds the optimizer).
//
// Both passes are HBM-bound (4 and 28 bytes per element); the arithmetic is float64 (the sum of squares so that
// total_norm is the correctly rounded float32 whatever the summation order, the update so that every stored value is
// rounded once) and stays far below the memory time: ~50 float64 instructions per element against 28 bytes.
// Deterministic: no atomics, no arrival counters, nothing to zero -- a captured launch needs no memset node.
// The descriptor table is read through the pointer the caller gives (device memory or device-addressable pinned host
// memory); each workgroup fetches its 64-byte descriptor once, into LDS.
#include "device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFinalThreads = 1024;
static_assert(sizeof(occd_optim_chunk) == 64, "one descriptor = one 64-byte fetch");

// The tensor pointers come out of the descriptor, so the compiler cannot see that they are global memory and would emit
// flat_ accesses (which also tick the LDS counter); the address-space qualifier makes them global_load / global_store.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float gcfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const f32x4 gcf32x4;

struct Hyper {
    const float* lr_dev;
    const float* norm_out;
    double lr, beta1, beta2, eps, weight_decay;
    // WINDOW kernels only: the position {first, last} of the micro-batch (device ints, or the host's when NULL), clipping on
    const int32_t* flags_dev;
    int32_t first, last, clip;
};

// The window position, loaded by one thread per flag and handed round through LDS (the caller's next __syncthreads
// publishes it): every branch on it is workgroup-uniform.
__device__ __forceinline__ void fetch_flags(const int32_t* flags_dev, int first, int last, int* s_flags) {
    if (threadIdx.x < 2) s_flags[threadIdx.x] = flags_dev ? flags_dev[threadIdx.x] : (threadIdx.x == 0 ? first : last);
}

__device__ __forceinline__ occd_optim_chunk fetch_chunk(const occd_optim_chunk* table, occd_optim_chunk* s_d) {
    if (threadIdx.x < 16)
        reinterpret_cast<uint32_t*>(s_d)[threadIdx.x] = reinterpret_cast<const uint32_t*>(table + blockIdx.x)[threadIdx.x];
    __syncthreads();
    return *s_d;
}

// sum over the workgroup, in a fixed order; the result is valid in thread 0
template <int NT>
__device__ __forceinline__ double block_sum(double x, double* s_red) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < NT / 64; ++w) t += s_red[w];
    return t;
}

// elements in front of the first 16-byte boundary (pointers are 4-byte aligned)
__device__ __forceinline__ int head_elems(gcfloat* p, int n) {
    const int h = (int)(((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u) >> 2);
    return h < n ? h : n;
}

template <bool ADVANCE_STEP>
__global__ void __launch_bounds__(kThreads) grad_sumsq_kernel(const occd_optim_chunk* __restrict__ table,
                                                              double* __restrict__ partials) {
    __shared__ occd_optim_chunk s_d;
    __shared__ double s_red[kThreads / 64];
    const occd_optim_chunk d = fetch_chunk(table, &s_d);
    const int tid = threadIdx.x, n = d.count;
    gcfloat* g = (gcfloat*)(d.g + d.offset);
    // the update pass (a later launch) reads the advanced counter; this pass does not read it
    if (ADVANCE_STEP && d.offset == 0 && tid == 0) *(gfloat*)d.step += 1.0f;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const int head = head_elems(g, n);
    if (tid < head) {
        const double x = (double)g[tid];
        a0 = x * x;
    }
    gcf32x4* g4 = (gcf32x4*)(g + head);
    const int n4 = (n - head) >> 2;
#pragma unroll 4
    for (int i = tid; i < n4; i += kThreads) {
        const f32x4 x = g4[i];
        a0 += (double)x.x * (double)x.x;
        a1 += (double)x.y * (double)x.y;
        a2 += (double)x.z * (double)x.z;
        a3 += (double)x.w * (double)x.w;
    }
    const int done = head + 4 * n4;
    if (tid < n - done) {
        const double x = (double)g[done + tid];
        a1 += x * x;
    }
    const double t = block_sum<kThreads>((a0 + a1) + (a2 + a3), s_red);
    if (tid == 0) partials[blockIdx.x] = t;
}

// `flags`: NULL, or the window position {first, last} of occd_accum_clip_adamw -- a micro-batch that does not close its
// window leaves norm_out as it is (one load per workgroup, and the grid is one workgroup)
__global__ void __launch_bounds__(kFinalThreads) norm_finalise_kernel(const double* __restrict__ partials, long n,
                                                                      float max_norm, float* __restrict__ norm_out,
                                                                      const int32_t* __restrict__ flags) {
    __shared__ double s_red[kFinalThreads / 64];
    __shared__ int s_last;
    if (threadIdx.x == 0) s_last = flags ? flags[1] : 1;
    __syncthreads();
    if (!s_last) return;
    double a = 0.0;
    for (long i = threadIdx.x; i < n; i += kFinalThreads) a += partials[i];
    const double t = block_sum<kFinalThreads>(a, s_red);
    if (threadIdx.x == 0) {
        const float total = (float)sqrt(t);
        // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0) on float32 tensors; clamp keeps a NaN
        const float c = max_norm / (total + 1e-6f);
        norm_out[0] = total;
        norm_out[1] = c > 1.0f ? 1.0f : c;
    }
}

struct Step {
    double coef, decay, one_m_b1, beta2, one_m_b2, step_size, bc2_sqrt, eps;
};

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const Step& s) {
    const double gd = (double)g * s.coef;
    double pd = (double)p * s.decay;
    const double md = (double)m + s.one_m_b1 * (gd - (double)m);
    const double vd = s.beta2 * (double)v + s.one_m_b2 * gd * gd;
    const double denom = sqrt(vd) / s.bc2_sqrt + s.eps;
    pd -= s.step_size * (md / denom);
    p = (float)pd;
    m = (float)md;
    v = (float)vd;
}

__device__ __forceinline__ void adamw_scalar(gfloat* p, gcfloat* g, gfloat* m, gfloat* v, int i, const Step& s) {
    float pc = p[i], mc = m[i], vc = v[i];
    adamw_one(pc, g[i], mc, vc, s);
    p[i] = pc;
    m[i] = mc;
    v[i] = vc;
}

// WINDOW: the gradient is the window's accumulator (d.acc, which shares p's offset to a 16-byte boundary); a micro-batch
// that does not close the window leaves before anything is read or written; without clipping the coefficient is exactly 1.
template <bool WINDOW>
__global__ void __launch_bounds__(kThreads) clip_adamw_kernel(const occd_optim_chunk* __restrict__ table, Hyper h) {
    __shared__ occd_optim_chunk s_d;
    __shared__ Step s_step;
    __shared__ int s_flags[2];
    if (WINDOW) fetch_flags(h.flags_dev, h.first, h.last, s_flags);
    const occd_optim_chunk d = fetch_chunk(table, &s_d);
    if (WINDOW && !s_flags[1]) return;
    const int tid = threadIdx.x, n = d.count;
    if (tid == 0) {
        const double lr = h.lr_dev ? (double)*h.lr_dev : h.lr;
        const double t = (double)*(gcfloat*)d.step;              // already advanced by the norm pass
        Step s;
        s.coef = (WINDOW && !h.clip) ? 1.0 : (double)h.norm_out[1];
        s.decay = 1.0 - lr * h.weight_decay;
        s.one_m_b1 = 1.0 - h.beta1;
        s.beta2 = h.beta2;
        s.one_m_b2 = 1.0 - h.beta2;
        s.step_size = lr / (1.0 - pow(h.beta1, t));
        s.bc2_sqrt = sqrt(1.0 - pow(h.beta2, t));
        s.eps = h.eps;
        s_step = s;
    }
    __syncthreads();
    const Step s = s_step;
    gfloat* p = (gfloat*)(d.p + d.offset);
    gfloat* m = (gfloat*)(d.m + d.offset);
    gfloat* v = (gfloat*)(d.v + d.offset);
    gcfloat* g = (gcfloat*)((WINDOW ? (const float*)d.acc : d.g) + d.offset);
    // 128-bit accesses where p, m and v share their offset to a 16-byte boundary (separately allocated tensors do); the
    // gradient -- a view at any float offset of a flat bucket -- joins them when it shares it too, else it is read by
    // dwords.  Chunk offsets are multiples of 8192 elements, so the tensors' base pointers decide.
    const uint32_t ap = (uint32_t)(uintptr_t)d.p & 15u;
    const bool vec = ap == ((uint32_t)(uintptr_t)d.m & 15u) && ap == ((uint32_t)(uintptr_t)d.v & 15u);
    const bool g_vec = ap == ((uint32_t)(uintptr_t)(WINDOW ? (const float*)d.acc : d.g) & 15u);
    const int head = vec ? head_elems(p, n) : n;
    for (int i = tid; i < head; i += kThreads) adamw_scalar(p, g, m, v, i, s);
    const int n4 = (n - head) >> 2;
    gf32x4* p4 = (gf32x4*)(p + head);
    gf32x4* m4 = (gf32x4*)(m + head);
    gf32x4* v4 = (gf32x4*)(v + head);
    gcfloat* gs = g + head;
#pragma unroll 2
    for (int i = tid; i < n4; i += kThreads) {
        f32x4 P = p4[i], M = m4[i], V = v4[i], G;
        if (g_vec) {
            G = ((gcf32x4*)gs)[i];
        } else {
            G.x = gs[4 * i];
            G.y = gs[4 * i + 1];
            G.z = gs[4 * i + 2];
            G.w = gs[4 * i + 3];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float pc = P[c], mc = M[c], vc = V[c];
            adamw_one(pc, G[c], mc, vc, s);
            P[c] = pc;
            M[c] = mc;
            V[c] = vc;
        }
        p4[i] = P;
        m4[i] = M;
        v4[i] = V;
    }
    for (int i = head + 4 * n4 + tid; i < n; i += kThreads) adamw_scalar(p, g, m, v, i, s);
}

// acc = [acc +] scale * g over one chunk, in float64 and rounded once.  The micro-batch that closes the window also leaves
// the chunk's sum of squares of the values it stored (from registers: the norm needs no second read) and advances `step`.
__device__ __forceinline__ float accum_one(float acc, float g, double scale, bool first, double& sq) {
    const double x = first ? scale * (double)g : (double)acc + scale * (double)g;
    const float r = (float)x;
    sq += (double)r * (double)r;
    return r;
}

__global__ void __launch_bounds__(kThreads) accum_kernel(const occd_optim_chunk* __restrict__ table,
                                                         double* __restrict__ partials, Hyper h, double scale) {
    __shared__ occd_optim_chunk s_d;
    __shared__ double s_red[kThreads / 64];
    __shared__ int s_flags[2];
    fetch_flags(h.flags_dev, h.first, h.last, s_flags);
    const occd_optim_chunk d = fetch_chunk(table, &s_d);
    const bool first = s_flags[0] != 0, last = s_flags[1] != 0;
    const int tid = threadIdx.x, n = d.count;
    gcfloat* g = (gcfloat*)(d.g + d.offset);
    gfloat* acc = (gfloat*)(d.acc + d.offset);
    // the update pass (a later launch) reads the advanced counter; this pass does not read it
    if (last && d.offset == 0 && tid == 0) *(gfloat*)d.step += 1.0f;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    // 128-bit accesses on acc; the gradient joins them when it shares acc's offset to a 16-byte boundary, else dwords
    const bool g_vec = ((uint32_t)(uintptr_t)d.acc & 15u) == ((uint32_t)(uintptr_t)d.g & 15u);
    const int head = head_elems(acc, n);
    if (tid < head) acc[tid] = accum_one(first ? 0.0f : acc[tid], g[tid], scale, first, a0);
    const int n4 = (n - head) >> 2;
    gf32x4* acc4 = (gf32x4*)(acc + head);
    gcfloat* gs = g + head;
#pragma unroll 2
    for (int i = tid; i < n4; i += kThreads) {
        f32x4 A = {0.0f, 0.0f, 0.0f, 0.0f}, G;
        if (!first) A = acc4[i];
        if (g_vec) {
            G = ((gcf32x4*)gs)[i];
        } else {
            G.x = gs[4 * i];
            G.y = gs[4 * i + 1];
            G.z = gs[4 * i + 2];
            G.w = gs[4 * i + 3];
        }
        A.x = accum_one(A.x, G.x, scale, first, a0);
        A.y = accum_one(A.y, G.y, scale, first, a1);
        A.z = accum_one(A.z, G.z, scale, first, a2);
        A.w = accum_one(A.w, G.w, scale, first, a3);
        acc4[i] = A;
    }
    const int done = head + 4 * n4;
    if (tid < n - done) acc[done + tid] = accum_one(first ? 0.0f : acc[done + tid], g[done + tid], scale, first, a1);
    if (!(last && h.clip)) return;                           // workgroup-uniform
    const double t = block_sum<kThreads>((a0 + a1) + (a2 + a3), s_red);
    if (tid == 0) partials[blockIdx.x] = t;
}

// The kernels dereference the table: device memory or device-addressable (pinned) host memory only.  The query is
// skipped while the stream is capturing (only stream calls are made inside a capture).
int check_table(const void* chunks, hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return OCCD_ELAUNCH;
    }
    if (cap != hipStreamCaptureStatusNone) return OCCD_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, chunks) != hipSuccess) {
        (void)hipGetLastError();
        return OCCD_EINVAL;
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeHost && attr.type != hipMemoryTypeManaged)
        return OCCD_EINVAL;
    return OCCD_OK;
}

int check_args(const occd_clip_adamw_args* a, hipStream_t st) {
    if (!a || !a->chunks || !a->partials || !a->norm_out) return OCCD_EINVAL;
    if (a->n_chunks <= 0 || a->n_chunks > 0x7FFFFFFFL || a->n_elems < 0 || !(a->max_norm > 0.0)) return OCCD_EINVAL;
    return check_table(a->chunks, st);
}

template <bool ADVANCE_STEP>
void launch_norm(const occd_clip_adamw_args* a, hipStream_t st) {
    occd::ProfScope prof("grad_sumsq", st, 2.0 * (double)a->n_elems, 4.0 * (double)a->n_elems + 72.0 * (double)a->n_chunks);
    hipLaunchKernelGGL(grad_sumsq_kernel<ADVANCE_STEP>, dim3((unsigned)a->n_chunks), dim3(kThreads), 0, st, a->chunks,
                       a->partials);
    hipLaunchKernelGGL(norm_finalise_kernel, dim3(1), dim3(kFinalThreads), 0, st, (const double*)a->partials,
                       (long)a->n_chunks, (float)a->max_norm, a->norm_out, (const int32_t*)nullptr);
}

}  // namespace

extern "C" int occd_grad_sumsq(const occd_clip_adamw_args* a, void* stream) {
    const int rc = check_args(a, (hipStream_t)stream);
    if (rc != OCCD_OK) return rc;
    launch_norm<false>(a, (hipStream_t)stream);
    return occd::check_launch();
}

extern "C" int occd_clip_adamw(const occd_clip_adamw_args* a, void* stream) {
    const int rc = check_args(a, (hipStream_t)stream);
    if (rc != OCCD_OK) return rc;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0) ||
        !(a->weight_decay >= 0.0) || (!a->lr_dev && !(a->lr >= 0.0)))
        return OCCD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    launch_norm<true>(a, st);
    Hyper h;
    h.lr_dev = a->lr_dev;
    h.norm_out = a->norm_out;
    h.lr = a->lr;
    h.beta1 = a->beta1;
    h.beta2 = a->beta2;
    h.eps = a->eps;
    h.weight_decay = a->weight_decay;
    h.flags_dev = nullptr;
    h.first = h.last = h.clip = 1;
    {
        occd::ProfScope prof("clip_adamw", st, 12.0 * (double)a->n_elems, 28.0 * (double)a->n_elems + 64.0 * (double)a->n_chunks);
        hipLaunchKernelGGL(clip_adamw_kernel<false>, dim3((unsigned)a->n_chunks), dim3(kThreads), 0, st, a->chunks, h);
    }
    return occd::check_launch();
}

extern "C" int occd_accum_clip_adamw(const occd_accum_adamw_args* a, void* stream) {
    if (!a || !a->chunks || a->n_chunks <= 0 || a->n_chunks > 0x7FFFFFFFL || a->n_elems < 0) return OCCD_EINVAL;
    const bool clip = a->max_norm > 0.0;
    if (clip && (!a->partials || !a->norm_out)) return OCCD_EINVAL;
    if (!(a->scale > 0.0) || !(a->scale <= 1.0)) return OCCD_EINVAL;
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0) ||
        !(a->weight_decay >= 0.0) || (!a->lr_dev && !(a->lr >= 0.0)))
        return OCCD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int rc = check_table(a->chunks, st);
    if (rc != OCCD_OK) return rc;
    Hyper h;
    h.lr_dev = a->lr_dev;
    h.norm_out = a->norm_out;
    h.lr = a->lr;
    h.beta1 = a->beta1;
    h.beta2 = a->beta2;
    h.eps = a->eps;
    h.weight_decay = a->weight_decay;
    h.flags_dev = a->flags_dev;
    h.first = a->first != 0;
    h.last = a->last != 0;
    h.clip = clip;
    const double ne = (double)a->n_elems, nc = (double)a->n_chunks;
    // with device flags every launch is enqueued (a captured graph has a fixed shape) and leaves early by itself;
    // with host flags the launches a non-closing micro-batch does not need are not made
    const bool may_close = a->flags_dev || h.last;
    {
        occd::ProfScope prof("grad_accum", st, 4.0 * ne, 12.0 * ne + 72.0 * nc);
        hipLaunchKernelGGL(accum_kernel, dim3((unsigned)a->n_chunks), dim3(kThreads), 0, st, a->chunks, a->partials, h, a->scale);
    }
    if (may_close && clip) {
        occd::ProfScope prof("grad_norm_finalise", st, nc, 8.0 * nc);
        hipLaunchKernelGGL(norm_finalise_kernel, dim3(1), dim3(kFinalThreads), 0, st, (const double*)a->partials,
                           (long)a->n_chunks, (float)a->max_norm, a->norm_out, a->flags_dev);
    }
    if (may_close) {
        occd::ProfScope prof("accum_adamw", st, 12.0 * ne, 28.0 * ne + 64.0 * nc);
        hipLaunchKernelGGL(clip_adamw_kernel<true>, dim3((unsigned)a->n_chunks), dim3(kThreads), 0, st, a->chunks, h);
    }
    return occd::check_launch();
}
