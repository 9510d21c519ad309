// K37: exact truncated squared Euclidean distance transform of label volumes (occd_edt_sq) and the distance-tolerant
// score counters made of it (occd_dist_metric).  Contract and definitions: include/occdepth_amd.h.
//
// D_s(v) = min(min over seeds u of slot s of |v - u|^2, T + 1) is separable: a pass along Z, then Y, then X, each
//   out[i] = min(min over |k| <= r of in[i + k] + k^2, T + 1),   r = floor(sqrt(T)),
// on values already clipped to T + 1.  A candidate further than r along an axis has k^2 > T, and a value that reached T + 1
// stays there under a saturating add, so the window never needs to be wider and the clip commutes with the passes.
// Everything is integer: the result does not depend on the schedule.
//
//   z_sweep_kernel   labels -> plane A.  The seeds of a slot are formed from the labels on the fly (no mask volume).  Along Z
//                    the input is 0 / infinity, so the pass is the distance to the nearest seed of the row: two sweeps per
//                    row in LDS (one thread per row, rows staged and written back coalesced), no window at all.
//   minplus_kernel   plane -> plane along N of a [outer][N][P] view with P contiguous (Y pass: N = Y, P = Z, outer = X;
//                    X pass: N = X, P = Y Z).  A workgroup stages TN + 2 r rows x 2 TPW columns in LDS (rows outside the
//                    axis and columns outside P are infinity), coalesced along P.  A thread owns one PAIR of columns,
//                    packed in 32 bits, and R = 8 consecutive rows: every LDS word it reads feeds 16 outputs through
//                    v_pk_add_u16 (clamped) and v_pk_min_u16 with a wave-uniform k^2: branch-free, (2 r + R) / R LDS reads
//                    and 2 packed operations per pair of outputs and k.
//   COUNT variant    the X pass of occd_dist_metric: D is not written but counted, for the voxels of the tile that are
//                    queries and belong to the slot, into a u32 LDS histogram (T + 2 bins) that is flushed with one 64-bit
//                    integer atomic per non-zero bin.  A tile without such a voxel ends before its window loop.
//
// No allocation, no host sync, no memset node: capture-safe.  The lower-envelope (parabola) form was not built: it is
// serial per row, and at the default T = 1024 the window is 65 wide against rows of 256.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kR = 8;                      // rows per thread of the min-plus passes
constexpr int kLdsBudget = 48 * 1024;       // bytes of dynamic LDS a workgroup may ask for
constexpr int kHistMaxBins = 4096;          // T + 2 above this: the counters are added to global memory directly
constexpr unsigned kInf = 0xFFFFu;

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pk_min_addsat(unsigned acc, unsigned v, unsigned ww) {
    const u16x2 s = __builtin_elementwise_add_sat(__builtin_bit_cast(u16x2, v), __builtin_bit_cast(u16x2, ww));
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, acc), s));
}

__device__ __forceinline__ int load_label(const void* base, int bytes, int64_t i) {
    return bytes == 1 ? (int)static_cast<const uint8_t*>(base)[i] : (int)static_cast<const uint16_t*>(base)[i];
}

// slot 0: every class 1 .. C - 1; slot c: class c (c < C, checked on the host)
__device__ __forceinline__ bool in_slot(int label, int slot, int C) {
    return slot == 0 ? (label >= 1 && label < C) : label == slot;
}

// Which volume an instance (blockIdx.y) takes its seeds from, and which slot.
//   edt:    instance = b S + i        -> vol[0] + b XYZ, slots[i]
//   metric: instance j of a chunk     -> g = inst0 + j, side = g / C, slot = g % C; side 0 takes the TARGET's seeds
struct Inst {
    const void* vol[2];
    int32_t bytes[2];
    int32_t metric, inst0, C, n_slots;
    int32_t slots[OCCD_EDT_MAX_CLASSES];
    int64_t frame;                                  // X Y Z
};

__device__ __forceinline__ void resolve(const Inst& in, int inst, const void*& vol, int& bytes, int64_t& off, int& slot) {
    if (in.metric) {
        const int g = in.inst0 + inst;
        const int side = g / in.C;
        slot = g - side * in.C;
        vol = in.vol[side];
        bytes = in.bytes[side];
        off = 0;
    } else {
        const int b = inst / in.n_slots;
        slot = in.slots[inst - b * in.n_slots];
        vol = in.vol[0];
        bytes = in.bytes[0];
        off = (int64_t)b * in.frame;
    }
}

struct ZP {
    Inst in;
    uint16_t* out;                                  // (instances, X Y, Z)
    int32_t rows, Z, zs, rows_per_block, T1;        // rows = X Y; zs: LDS row stride in u16 (zs / 2 odd)
};

// distance to the nearest seed of the row, squared and clipped; STAGED: through LDS, else in place in global memory (rows
// too long for LDS: a thread walks its own row, uncoalesced)
template <bool STAGED>
__global__ __launch_bounds__(kThreads) void z_sweep_kernel(ZP p) {
    extern __shared__ uint32_t smem[];
    uint16_t* tile = reinterpret_cast<uint16_t*>(smem);
    const void* vol; int bytes, slot; int64_t off;
    resolve(p.in, blockIdx.y, vol, bytes, off, slot);
    const int Z = p.Z, C = p.in.C;
    const int row0 = blockIdx.x * p.rows_per_block;
    const int nrows = min(p.rows_per_block, p.rows - row0);          // row0 < rows for every workgroup
    const int64_t src = off + (int64_t)row0 * Z;
    uint16_t* dst = p.out + (int64_t)blockIdx.y * p.in.frame + (int64_t)row0 * Z;
    if (STAGED) {
        const int n = nrows * Z;                                      // <= rows_per_block * Z, which fits the LDS budget
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int r = i / Z;
            tile[r * p.zs + (i - r * Z)] = in_slot(load_label(vol, bytes, src + i), slot, C) ? 0 : kInf;
        }
        __syncthreads();
    }
    if ((int)threadIdx.x < nrows) {
        const int t = threadIdx.x;
        unsigned d = kInf;                                            // distance to the last seed seen, saturating
        for (int z = 0; z < Z; ++z) {
            const bool seed = STAGED ? tile[t * p.zs + z] == 0 : in_slot(load_label(vol, bytes, src + (int64_t)t * Z + z), slot, C);
            d = seed ? 0u : min(d + 1u, kInf);
            if (STAGED) tile[t * p.zs + z] = (uint16_t)d; else dst[(int64_t)t * Z + z] = (uint16_t)d;
        }
        d = kInf;
        for (int z = Z - 1; z >= 0; --z) {
            const unsigned f = STAGED ? tile[t * p.zs + z] : dst[(int64_t)t * Z + z];
            d = f == 0u ? 0u : min(d + 1u, kInf);
            const unsigned m = min(f, d);
            const unsigned v = m >= 256u ? (unsigned)p.T1 : min(m * m, (unsigned)p.T1);   // 256^2 > any T
            if (STAGED) tile[t * p.zs + z] = (uint16_t)v; else dst[(int64_t)t * Z + z] = (uint16_t)v;
        }
    }
    if (STAGED) {
        __syncthreads();
        const int n = nrows * Z;
        for (int i = threadIdx.x; i < n; i += kThreads) {
            const int r = i / Z;
            dst[i] = tile[r * p.zs + (i - r * Z)];
        }
    }
}

struct MP {
    const uint16_t* in;                             // (instances, outer, N, P)
    uint16_t* out;                                  // the same layout (not read or written by the COUNT variant)
    int32_t N, P, outer, r, T1;
    int32_t tpw_log2, tn, n_row_tiles, n_col_tiles; // tile: tn rows x 2^(tpw_log2 + 1) columns
    int64_t frame;                                  // outer N P = X Y Z
    // COUNT
    const void* pred;                               // this frame's volumes
    const void* target;
    const uint8_t* mask;
    unsigned long long* counts;
    int32_t pred_bytes, target_bytes, C, inst0, lds_hist;
};

template <bool COUNT>
__global__ __launch_bounds__(kThreads) void minplus_kernel(MP p) {
    extern __shared__ uint32_t smem[];
    const int tpw = 1 << p.tpw_log2, cols = tpw * 2, r = p.r, N = p.N, P = p.P;
    const int rows_l = p.tn + 2 * r;
    int bid = blockIdx.x;
    const int ct = bid % p.n_col_tiles; bid /= p.n_col_tiles;
    const int rt = bid % p.n_row_tiles; bid /= p.n_row_tiles;        // bid: the outer index now
    const int inst = blockIdx.y;
    const uint16_t* src = p.in + (int64_t)inst * p.frame + (int64_t)bid * N * P;
    const int row0 = rt * p.tn, col0 = ct * cols;
    const int cp = threadIdx.x & (tpw - 1), i0 = (threadIdx.x >> p.tpw_log2) * kR;

    // COUNT: which of this thread's 2 kR voxels are queries of the instance's side that belong to its slot
    unsigned member = 0u;
    int slot = 0, side = 0;
    uint32_t* hist = smem + rows_l * tpw;
    if (COUNT) {
        const int g = p.inst0 + inst;
        side = g / p.C;
        slot = g - side * p.C;
        for (int q = 0; q < kR; ++q) {
            const int gi = row0 + i0 + q;
            for (int h = 0; h < 2; ++h) {
                const int gc = col0 + 2 * cp + h;
                if (gi < N && gc < P) {
                    const int64_t v = (int64_t)gi * P + gc;                      // outer == 1: the voxel of the frame
                    const int tl = load_label(p.target, p.target_bytes, v);
                    if (tl != 255 && (!p.mask || p.mask[v])) {
                        const int ml = side == 0 ? load_label(p.pred, p.pred_bytes, v) : tl;
                        if (in_slot(ml, slot, p.C)) member |= 1u << (2 * q + h);
                    }
                }
            }
        }
        if (!__syncthreads_or(member != 0u)) return;                             // nothing to count in this tile
        if (p.lds_hist)
            for (int i = threadIdx.x; i < p.T1 + 1; i += kThreads) hist[i] = 0u;
    }

    uint16_t* t16 = reinterpret_cast<uint16_t*>(smem);
    const int n = rows_l * cols;
    for (int i = threadIdx.x; i < n; i += kThreads) {
        const int gr = row0 - r + (i >> (p.tpw_log2 + 1)), gc = col0 + (i & (cols - 1));
        t16[i] = (gr >= 0 && gr < N && gc < P) ? src[(int64_t)gr * P + gc] : (uint16_t)kInf;
    }
    __syncthreads();

    unsigned acc[kR];
#pragma unroll
    for (int q = 0; q < kR; ++q) acc[q] = 0xFFFFFFFFu;
    const uint32_t* col = smem + i0 * tpw + cp;                                  // rows i0 .. i0 + 2 r + kR - 1 < rows_l
    for (int d = 0; d < 2 * r + kR; ++d) {
        const unsigned v = col[d * tpw];
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const int k = d - r - q;                                             // wave-uniform; |k| > r only adds values > T
            const unsigned w = min((unsigned)(k * k), kInf);
            acc[q] = pk_min_addsat(acc[q], v, w | (w << 16));
        }
    }

    const unsigned T1 = (unsigned)p.T1;
    if (!COUNT) {
        uint16_t* dst = p.out + (int64_t)inst * p.frame + (int64_t)bid * N * P;
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const int gi = row0 + i0 + q, gc = col0 + 2 * cp;
            if (gi < N) {
                if (gc < P) dst[(int64_t)gi * P + gc] = (uint16_t)min(acc[q] & 0xFFFFu, T1);
                if (gc + 1 < P) dst[(int64_t)gi * P + gc + 1] = (uint16_t)min(acc[q] >> 16, T1);
            }
        }
    } else {
        unsigned long long* out = p.counts + (int64_t)(side * p.C + slot) * (p.T1 + 1);
#pragma unroll
        for (int q = 0; q < kR; ++q) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (member & (1u << (2 * q + h))) {
                    const unsigned dist = min(h ? acc[q] >> 16 : acc[q] & 0xFFFFu, T1);   // a bin 0 .. T + 1
                    if (p.lds_hist) atomicAdd(&hist[dist], 1u);
                    else atomicAdd(&out[dist], 1ull);
                }
            }
        }
        if (p.lds_hist) {
            __syncthreads();
            for (int i = threadIdx.x; i < p.T1 + 1; i += kThreads)
                if (hist[i]) atomicAdd(&out[i], (unsigned long long)hist[i]);
        }
    }
}

int isqrt(int t) {
    int r = 0;
    while ((r + 1) * (r + 1) <= t) ++r;
    return r;
}

bool common_checks(const OccdEdtArgs* a) {
    if (a->batch <= 0 || a->X <= 0 || a->Y <= 0 || a->Z <= 0) return false;
    if (a->label_bytes != 1 && a->label_bytes != 2) return false;
    if (a->n_classes < 1 || a->n_classes > OCCD_EDT_MAX_CLASSES) return false;
    if (a->max_d2 < 1 || a->max_d2 > 65534) return false;
    const int64_t X = a->X, Y = a->Y, Z = a->Z, lim = (int64_t)1 << 31;
    if (X >= 65536 || Y >= 65536 || Z >= 65536) return false;                   // squares below stay in 64 bits
    if (X * X + Y * Y + Z * Z >= lim) return false;
    if (X * Y >= lim || X * Y * Z >= lim || X * Y * Z * a->batch >= lim) return false;
    return true;
}

// the three passes over `instances` volumes of one frame size: labels -> A (z), A -> B (y), B -> `last` (x; COUNT: counters)
int run_passes(const Inst& in, int instances, int X, int Y, int Z, int T, uint16_t* A, uint16_t* B, uint16_t* last, MP* count,
               hipStream_t s) {
    const int r = isqrt(T);
    ZP z;
    z.in = in; z.out = A; z.rows = X * Y; z.Z = Z; z.T1 = T + 1;
    z.zs = (Z + 1) & ~1;
    if (!((z.zs >> 1) & 1)) z.zs += 2;                                           // zs / 2 odd: rows fall into different banks
    const bool staged = (int64_t)z.zs * 2 <= kLdsBudget;
    z.rows_per_block = staged ? (int)std::min<int64_t>(kThreads, kLdsBudget / (z.zs * 2)) : kThreads;
    const int64_t zblocks = ((int64_t)z.rows + z.rows_per_block - 1) / z.rows_per_block;
    if (instances > 65535) return OCCD_EINVAL;
    const double plane = 2.0 * instances * (double)in.frame;                     // bytes of one set of uint16 planes
    {
        occd::ProfScope prof(count ? "dist_metric_z" : "edt_sq_z", s, 0.0, plane);
        const dim3 grid((unsigned)zblocks, (unsigned)instances);
        if (staged) hipLaunchKernelGGL(z_sweep_kernel<true>, grid, dim3(kThreads), (size_t)z.rows_per_block * z.zs * 2, s, z);
        else hipLaunchKernelGGL(z_sweep_kernel<false>, grid, dim3(kThreads), 0, s, z);
    }
    for (int pass = 0; pass < 2; ++pass) {
        MP m;
        if (count && pass == 1) m = *count; else m = MP();
        m.N = pass == 0 ? Y : X;
        m.P = pass == 0 ? Z : Y * Z;
        m.outer = pass == 0 ? X : 1;
        m.frame = in.frame;
        m.r = std::min(r, m.N - 1);
        m.T1 = T + 1;
        m.in = pass == 0 ? A : B;
        m.out = pass == 0 ? B : last;
        const bool counting = count && pass == 1;
        const int hist_bytes = counting && m.lds_hist ? (T + 2) * 4 : 0;
        // 64 columns x 64 rows per workgroup where the columns exist and the halo fits, else 32 columns x 128 rows
        m.tpw_log2 = (m.P > 32 && (64 + 2 * m.r) * 32 * 4 + hist_bytes <= kLdsBudget) ? 5 : 4;
        const int tpw = 1 << m.tpw_log2;
        m.tn = (kThreads / tpw) * kR;
        const size_t lds = (size_t)(m.tn + 2 * m.r) * tpw * 4 + hist_bytes;       // r <= 255: at most (128 + 510) 64 + 16392 bytes
        m.n_row_tiles = (m.N + m.tn - 1) / m.tn;
        m.n_col_tiles = (m.P + 2 * tpw - 1) / (2 * tpw);
        const int64_t blocks = (int64_t)m.n_row_tiles * m.n_col_tiles * m.outer;
        if (blocks >= ((int64_t)1 << 31)) return OCCD_EINVAL;
        const dim3 grid((unsigned)blocks, (unsigned)instances);
        occd::ProfScope prof(count ? (pass ? "dist_metric_x" : "dist_metric_y") : (pass ? "edt_sq_x" : "edt_sq_y"), s, 0.0,
                             counting ? plane : 2.0 * plane);
        if (counting) hipLaunchKernelGGL(minplus_kernel<true>, grid, dim3(kThreads), lds, s, m);
        else hipLaunchKernelGGL(minplus_kernel<false>, grid, dim3(kThreads), lds, s, m);
    }
    return 0;
}

}  // namespace

extern "C" int occd_edt_sq(const OccdEdtArgs* a, void* stream) {
    if (!a || !a->labels || !a->dist || !a->scratch) return OCCD_EINVAL;
    if (!common_checks(a)) return OCCD_EINVAL;
    if (a->n_slots < 1 || a->n_slots > OCCD_EDT_MAX_CLASSES) return OCCD_EINVAL;
    for (int i = 0; i < a->n_slots; ++i)
        if (a->slots[i] < 0 || a->slots[i] >= a->n_classes) return OCCD_EINVAL;
    const int64_t frame = (int64_t)a->X * a->Y * a->Z;
    const int64_t instances = (int64_t)a->batch * a->n_slots;
    if (instances > 65535 || instances * frame >= ((int64_t)1 << 40)) return OCCD_EINVAL;
    if (a->scratch_bytes < instances * frame * 2) return OCCD_EINVAL;
    Inst in = Inst();
    in.vol[0] = a->labels; in.bytes[0] = a->label_bytes;
    in.metric = 0; in.C = a->n_classes; in.n_slots = a->n_slots; in.frame = frame;
    for (int i = 0; i < a->n_slots; ++i) in.slots[i] = a->slots[i];
    hipStream_t s = (hipStream_t)stream;
    occd::ProfScope prof("edt_sq", s, 0.0, (double)a->batch * frame * a->label_bytes + 2.0 * instances * frame);
    const int rc = run_passes(in, (int)instances, a->X, a->Y, a->Z, a->max_d2, a->dist, static_cast<uint16_t*>(a->scratch),
                              a->dist, nullptr, s);
    return rc ? rc : occd::check_launch();
}

extern "C" int occd_dist_metric(const OccdEdtArgs* a, void* stream) {
    if (!a || !a->labels || !a->target || !a->counts || !a->scratch) return OCCD_EINVAL;
    if (!common_checks(a)) return OCCD_EINVAL;
    if (a->target_bytes != 1 && a->target_bytes != 2) return OCCD_EINVAL;
    const int64_t frame = (int64_t)a->X * a->Y * a->Z;
    if (a->scratch_bytes < 2 * (int64_t)OCCD_EDT_CHUNK * frame * 2) return OCCD_EINVAL;
    const int C = a->n_classes, T = a->max_d2;
    uint16_t* A = static_cast<uint16_t*>(a->scratch);
    uint16_t* B = A + (int64_t)OCCD_EDT_CHUNK * frame;
    hipStream_t s = (hipStream_t)stream;
    occd::ProfScope prof("dist_metric", s, 0.0, (double)a->batch * frame * (a->label_bytes + a->target_bytes + (a->mask ? 1 : 0)));
    for (int b = 0; b < a->batch; ++b) {
        const void* pred = static_cast<const char*>(a->labels) + (int64_t)b * frame * a->label_bytes;
        const void* target = static_cast<const char*>(a->target) + (int64_t)b * frame * a->target_bytes;
        for (int c0 = 0; c0 < 2 * C; c0 += OCCD_EDT_CHUNK) {
            Inst in = Inst();
            in.vol[0] = target; in.bytes[0] = a->target_bytes;       // side 0: prediction queries, the target's seeds
            in.vol[1] = pred; in.bytes[1] = a->label_bytes;          // side 1: target queries, the prediction's seeds
            in.metric = 1; in.inst0 = c0; in.C = C; in.frame = frame;
            MP m = MP();
            m.pred = pred; m.target = target; m.mask = a->mask ? a->mask + (int64_t)b * frame : nullptr;
            m.counts = reinterpret_cast<unsigned long long*>(a->counts);
            m.pred_bytes = a->label_bytes; m.target_bytes = a->target_bytes; m.C = C; m.inst0 = c0;
            m.lds_hist = T + 2 <= kHistMaxBins;
            const int rc = run_passes(in, std::min((int)OCCD_EDT_CHUNK, 2 * C - c0), a->X, a->Y, a->Z, T, A, B, nullptr, &m, s);
            if (rc) return rc;
        }
    }
    return occd::check_launch();
}
