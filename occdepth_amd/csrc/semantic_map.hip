// K30: the sequence-level semantic map (occd_map_integrate, occd_map_brick_labels, occd_map_count, occd_map_extract), and
// K32: the map read back into a frame's voxels (occd_map_sample), and
// K33: the counter-wise saturating sum of two sets of bricks (occd_map_merge).
// Contract: include/occdepth_amd.h.
//
// The map is a pool of 16^3 bricks of unsigned 16-bit vote counters, one row of `pitch` counters per voxel, row
// (i*16 + j)*16 + l of its brick.  The host (semantic_map.py) keeps the directory key -> slot and hands every launch a
// table with one row per brick; a workgroup takes one table row, so a counter has exactly one owner per launch: no
// atomics anywhere, and the bytes written do not depend on the schedule.
//
// Integrate is a gather: every voxel of every touched brick computes, in int32 fixed point, the frame voxel it falls
// into, reads that label and increments one counter.  The 256 threads of a workgroup are the (j, l) plane of the brick
// and every thread walks i: at one step the workgroup touches 256 CONSECUTIVE vote rows (a wave 64, i.e. 64 * pitch * 2
// contiguous bytes, whole 128-byte lines), and the 16 lanes of a z-run read labels that are consecutive in the frame
// under a pure yaw and near each other under the small pitch / roll of driving.  (A thread per z-run, the other natural
// assignment, puts the lanes of a wave 16 rows apart: every load instruction then touches 64 different lines.  Measured in
// a probe build at 256 x 256 x 32 x 20: 0.052 against 0.031 ms with the counters in the Infinity Cache, 0.081 against
// 0.043 ms from HBM, the same votes -- DESIGN.md K30.)
//
// Extraction reads every row in 8-byte pieces.  The compacted list is count per brick -> exclusive scan (the caller's)
// -> ordered write: inside a workgroup the 4096 voxels go in 16 passes of 256, a wave orders its lanes with a ballot and
// mbcnt, the waves hand their totals over through LDS (two buffers, one barrier per pass).
//
// Weighted votes (occd_map_integrate_weighted, occd_map_sample_weighted) are the same two kernels instantiated with
// WEIGHTED = true: a byte of weight per frame voxel where the unweighted form has a yes / no mask.
#include <stddef.h>
#include <string.h>

#include "common.h"
#include "device.h"

namespace {

constexpr int kBrick = OCCD_MAP_BRICK;
constexpr int kBrickVox = kBrick * kBrick * kBrick;     // 4096
constexpr int kThreads = kBrick * kBrick;               // 256: the (j, l) plane, or one pass of the extraction
constexpr int64_t kMaxVox = (int64_t)1 << 28;           // flat frame indices stay far inside int32
constexpr int64_t kMaxCells = (int64_t)1 << 27;         // directory entries of a sample window
static_assert(kBrick == 16, "the thread layouts below are written for 16^3 bricks");

template <int BYTES>
__device__ __forceinline__ uint32_t load_label(const void* base, uint32_t n) {
    if (BYTES == 1) return static_cast<const uint8_t*>(base)[n];
    return static_cast<const uint16_t*>(base)[n];
}

// WEIGHTED (occd_map_integrate_weighted): a.mask is the required weight volume, the vote counts weight[n] and the counter
// saturates at 65535; otherwise a.mask is the optional yes / no mask and a vote counts one
template <int LB, bool WEIGHTED>
__global__ void __launch_bounds__(kThreads) map_integrate_kernel(const OccdMapFrameArgs a) {
    const int32_t* row = a.table + (size_t)blockIdx.x * 16;
    const int32_t slot = row[0];
    if (slot < 0 || slot >= a.capacity) return;         // the whole workgroup: a row without a brick in the pool
    const int tid = threadIdx.x;
    const uint32_t j = (uint32_t)tid >> 4, l = (uint32_t)tid & 15u;
    // unsigned arithmetic wraps; the host keeps |gq| < 2^31, and whatever a bad table holds is range-checked below
    uint32_t gq[3], step[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        step[r] = (uint32_t)row[4 + 3 * r];
        gq[r] = (uint32_t)row[4 + 3 * r + 1] * j + (uint32_t)row[4 + 3 * r + 2] * l + (uint32_t)row[13 + r];
    }
    uint16_t* rows = a.votes + ((size_t)slot * kBrickVox + (size_t)tid) * (size_t)a.pitch;
    for (int i = 0; i < kBrick; ++i) {
        const int32_t ix = (int32_t)gq[0] >> 16, iy = (int32_t)gq[1] >> 16, iz = (int32_t)gq[2] >> 16;
#pragma unroll
        for (int r = 0; r < 3; ++r) gq[r] += step[r];
        if (ix < 0 || ix >= a.X || iy < 0 || iy >= a.Y || iz < 0 || iz >= a.Z) continue;
        const uint32_t n = ((uint32_t)ix * (uint32_t)a.Y + (uint32_t)iy) * (uint32_t)a.Z + (uint32_t)iz;   // < X Y Z <= 2^28
        uint32_t w = 1u;
        if (WEIGHTED) {
            w = a.mask[n];
            if (w == 0u) continue;
        } else if (a.mask != nullptr && a.mask[n] == 0) continue;
        const uint32_t label = load_label<LB>(a.labels, n);
        if (label >= (uint32_t)a.C) continue;           // C <= pitch: the counter lies inside the row
        uint16_t* c = rows + (size_t)i * kThreads * (size_t)a.pitch + label;
        const uint16_t v = *c;
        if (WEIGHTED) {
            const uint32_t sum = (uint32_t)v + w;
            if (v != 0xffffu) *c = (uint16_t)(sum < 0xffffu ? sum : 0xffffu);
        } else if (v != 0xffffu) *c = (uint16_t)(v + 1);
    }
}

// argmax (the lowest class on a tie) and sum of the C counters of one row, read in 8-byte pieces.  The counter of class
// `dec` counts one less unless it is 0 or 65535 (sample's exclude_self; ~0u: none); best = the maximum, at = the counter
// of class `ask` (0 when there is no such class).  WEIGHTED (occd_map_sample_weighted): the counter of class `dec` counts
// `amount` (> 0) less unless it is 65535 or below `amount` -- for amount = 1 the same rule
template <bool WEIGHTED = false>
__device__ __forceinline__ void decide(const uint16_t* row, int C, uint32_t dec, uint32_t ask, uint32_t& label, uint32_t& nobs,
                                       uint32_t& best, uint32_t& at, uint32_t amount = 1u) {
    const u32x2* q = reinterpret_cast<const u32x2*>(row);
    best = 0;
    label = 0;
    nobs = 0;
    at = 0;
    const int nq = (C + 3) >> 2;                        // <= 8, and 4 nq <= pitch
    for (int k = 0; k < nq; ++k) {
        const u32x2 w = q[k];
        const uint32_t v[4] = {w.x & 0xffffu, w.x >> 16, w.y & 0xffffu, w.y >> 16};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * k + e;
            if (c < C) {
                const uint32_t n = WEIGHTED ? v[e] - ((uint32_t)c == dec && v[e] != 0xffffu && v[e] >= amount ? amount : 0u)
                                            : v[e] - (uint32_t)((uint32_t)c == dec && v[e] != 0u && v[e] != 0xffffu);
                nobs += n;
                if ((uint32_t)c == ask) at = n;
                if (n > best) { best = n; label = (uint32_t)c; }
            }
        }
    }
}

__device__ __forceinline__ void decide(const uint16_t* row, int C, uint32_t& label, uint32_t& nobs) {
    uint32_t best, at;
    decide(row, C, ~0u, ~0u, label, nobs, best, at);
}

__global__ void __launch_bounds__(kThreads) map_brick_labels_kernel(const OccdMapExtractArgs a) {
    const int32_t slot = a.table[(size_t)blockIdx.x * 4];
    const bool have = slot >= 0 && slot < a.capacity;
    uint8_t* out = a.dense + (size_t)blockIdx.x * kBrickVox;
    for (int pass = 0; pass < kBrickVox / kThreads; ++pass) {
        const int v = pass * kThreads + (int)threadIdx.x;
        uint32_t label = 255u, nobs = 0;
        if (have) decide(a.votes + ((size_t)slot * kBrickVox + (size_t)v) * (size_t)a.pitch, a.C, label, nobs);
        out[v] = (uint8_t)(nobs ? label : 255u);
    }
}

// WRITE = false: counts[brick]; WRITE = true: the ordered write behind offsets[brick]
template <bool WRITE>
__global__ void __launch_bounds__(kThreads) map_scan_kernel(const OccdMapExtractArgs a) {
    __shared__ int wave_n[2][kThreads / 64];
    const int32_t* row = a.table + (size_t)blockIdx.x * 4;
    const int32_t slot = row[0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (slot < 0 || slot >= a.capacity) {               // the whole workgroup: not in the map, nothing kept
        if (!WRITE && tid == 0) a.counts[blockIdx.x] = 0;
        return;
    }
    const uint32_t need = a.min_obs > 1 ? (uint32_t)a.min_obs : 1u;
    int64_t out = WRITE ? a.offsets[blockIdx.x] : 0;
    int total = 0;
    for (int pass = 0; pass < kBrickVox / kThreads; ++pass) {
        const int v = pass * kThreads + tid;
        uint32_t label, nobs;
        decide(a.votes + ((size_t)slot * kBrickVox + (size_t)v) * (size_t)a.pitch, a.C, label, nobs);
        const bool keep = nobs >= need && (a.include_empty != 0 || label != 0u);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_n[pass & 1][wave] = __popcll(m);
        __syncthreads();                                // the other buffer is free: every wave passed the previous barrier
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) {
            const int n = wave_n[pass & 1][w];
            all += n;
            before += w < wave ? n : 0;
        }
        if (WRITE && keep) {
            const int64_t pos = out + before +
                (int64_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (pos >= 0 && pos < a.n_out) {            // offsets that do not belong to these counts write nothing
                const uint32_t i = (uint32_t)v >> 8, j = ((uint32_t)v >> 4) & 15u, l = (uint32_t)v & 15u;
                a.coords[pos * 3 + 0] = (int32_t)((uint32_t)row[1] * (uint32_t)kBrick + i);
                a.coords[pos * 3 + 1] = (int32_t)((uint32_t)row[2] * (uint32_t)kBrick + j);
                a.coords[pos * 3 + 2] = (int32_t)((uint32_t)row[3] * (uint32_t)kBrick + l);
                a.labels[pos] = (uint8_t)label;
                a.n_obs[pos] = (uint16_t)(nobs < 0xffffu ? nobs : 0xffffu);
            }
        }
        out += all;
        total += all;
    }
    if (!WRITE && tid == 0) a.counts[blockIdx.x] = total;
}

// K32: one thread per frame voxel, z fastest.  The transposed access pattern of integrate: there a brick's (j, l) plane
// reads labels that are scattered over the frame, here a z-column of the frame reads vote rows -- under a pure yaw z runs
// along the brick's l, so the 16 lanes of a z-run read 16 consecutive rows (16 * pitch * 2 contiguous bytes, 640 at pitch
// 20) and a wave touches as few 128-byte lines per load as the frame's heading allows; labels and n_obs are written
// coalesced.  (A thread per (x, y) column walking z puts the lanes of a wave 16 rows or more apart, the argument of
// integrate's header with the roles swapped.)
// WEIGHTED (occd_map_sample_weighted): a.own_mask is the weight volume the frame voted with, and exclude_self retracts that
// weight
template <int LB, bool WEIGHTED>
__global__ void __launch_bounds__(kThreads) map_sample_kernel(const OccdMapSampleArgs a) {
    const uint32_t S = (uint32_t)a.X * (uint32_t)a.Y * (uint32_t)a.Z;          // <= 2^28
    const uint32_t n = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (n >= S) return;
    const uint32_t z = n % (uint32_t)a.Z, xy = n / (uint32_t)a.Z;
    const uint32_t y = xy % (uint32_t)a.Y, x = xy / (uint32_t)a.Y;
    // unsigned arithmetic wraps; the host keeps |wq| < 2^31, and whatever bad coefficients give is range-checked below
    int32_t cell[3];
    uint32_t loc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint32_t wq = (uint32_t)a.Bq[3 * r] * x + (uint32_t)a.Bq[3 * r + 1] * y + (uint32_t)a.Bq[3 * r + 2] * z + (uint32_t)a.dq[r];
        const int32_t idx = (int32_t)wq >> 16;
        cell[r] = idx >> 4;
        loc[r] = (uint32_t)idx & 15u;
    }
    const uint32_t own = a.own != nullptr ? load_label<LB>(a.own, n) : 255u;
    uint32_t label = 0, nobs = 0;
    if (cell[0] >= 0 && cell[0] < a.gx && cell[1] >= 0 && cell[1] < a.gy && cell[2] >= 0 && cell[2] < a.gz) {
        const int32_t r = a.cells[((size_t)cell[0] * (size_t)a.gy + (size_t)cell[1]) * (size_t)a.gz + (size_t)cell[2]];
        if (r >= 0 && r < a.n_bricks) {
            const int32_t* row = a.table + (size_t)r * 16;
            const int32_t slot = row[0];
            if (slot >= 0 && slot < a.capacity) {
                uint32_t dec = ~0u, amount = 1u;
                if (a.flags & OCCD_MAP_SAMPLE_EXCLUDE_SELF) {              // the frame voxel integrate maps this world voxel to
                    int32_t g[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const uint32_t gq = (uint32_t)row[4 + 3 * k] * loc[0] + (uint32_t)row[4 + 3 * k + 1] * loc[1] +
                                            (uint32_t)row[4 + 3 * k + 2] * loc[2] + (uint32_t)row[13 + k];
                        g[k] = (int32_t)gq >> 16;
                    }
                    if (g[0] >= 0 && g[0] < a.X && g[1] >= 0 && g[1] < a.Y && g[2] >= 0 && g[2] < a.Z) {
                        const uint32_t m = ((uint32_t)g[0] * (uint32_t)a.Y + (uint32_t)g[1]) * (uint32_t)a.Z + (uint32_t)g[2];
                        if (WEIGHTED) amount = a.own_mask[m];              // required under this flag (the entry point checks)
                        if (WEIGHTED ? amount != 0u : (a.own_mask == nullptr || a.own_mask[m] != 0)) {
                            const uint32_t voted = load_label<LB>(a.own, m);
                            if (voted < (uint32_t)a.C) dec = voted;
                        }
                    }
                }
                const uint32_t v = (loc[0] * kBrick + loc[1]) * kBrick + loc[2];
                uint32_t best, at;
                decide<WEIGHTED>(a.votes + ((size_t)slot * kBrickVox + (size_t)v) * (size_t)a.pitch, a.C, dec, own, label, nobs, best, at,
                                 amount);
                if ((a.flags & OCCD_MAP_SAMPLE_KEEP_OWN) && own < (uint32_t)a.C && at == best && best > 0u) label = own;
            }
        }
    }
    const uint32_t need = a.min_obs > 1 ? (uint32_t)a.min_obs : 1u;
    a.labels[n] = (uint8_t)(nobs >= need ? label : (own < 255u ? own : 255u));
    a.n_obs[n] = (uint16_t)(nobs < 0xffffu ? nobs : 0xffffu);
}

// K33: dst = min(dst + src, 65535) over the bricks a table pairs up.  A brick is 512 * pitch 16-byte pieces and nothing
// in it depends on anything but the same piece of the other operand, so this is a stream: a workgroup takes a 1 / split
// part of one table row (blockIdx.x = row, blockIdx.y = part; whole multiples of 256 pieces), a thread takes pieces
// 256 apart (a wave reads 1 KiB contiguous per load), issues the 2 * kMergeUnroll 16-byte loads of a round before the
// first add, and adds two counters per 32-bit lane with the packed clamped add.  Every counter has one owner.
constexpr int kMergeUnroll = 4;
constexpr int kMergeSplit = 8;                          // parts per brick when the caller does not ask, for a launch of fewer
constexpr int kMergeWhole = 1024;                       // bricks than this; whole bricks from there on (measured: DESIGN.md K33)
typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t add_sat_u16x2(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_add_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

__global__ void __launch_bounds__(kThreads) map_merge_kernel(const OccdMapMergeArgs a, const int pieces) {
    const int32_t* row = a.table + (size_t)blockIdx.x * 2;
    const int32_t slot = row[0], from = row[1];
    if (slot < 0 || slot >= a.capacity || from < 0 || from >= a.src_capacity) return;      // the whole workgroup
    const size_t brick = (size_t)kBrickVox / 8 * (size_t)a.pitch;                          // 16-byte pieces per brick
    const size_t part = (size_t)blockIdx.y * (size_t)pieces + threadIdx.x;
    u32x4* dst = reinterpret_cast<u32x4*>(a.votes) + (size_t)slot * brick + part;
    const u32x4* src = reinterpret_cast<const u32x4*>(a.src) + (size_t)from * brick + part;
    for (int base = 0; base < pieces; base += kMergeUnroll * kThreads) {
        u32x4 d[kMergeUnroll], s[kMergeUnroll];
#pragma unroll
        for (int u = 0; u < kMergeUnroll; ++u) {
            const int p = base + u * kThreads;          // pieces is a multiple of 256: p < pieces holds for a whole workgroup
            if (p < pieces) {
                d[u] = dst[p];
                s[u] = __builtin_nontemporal_load(src + p);
            }
        }
#pragma unroll
        for (int u = 0; u < kMergeUnroll; ++u) {
            const int p = base + u * kThreads;
            if (p < pieces) {
                u32x4 r;
                r.x = add_sat_u16x2(d[u].x, s[u].x);
                r.y = add_sat_u16x2(d[u].y, s[u].y);
                r.z = add_sat_u16x2(d[u].z, s[u].z);
                r.w = add_sat_u16x2(d[u].w, s[u].w);
                dst[p] = r;
            }
        }
    }
}

bool pool_ok(const void* votes, const int32_t* table, int32_t n_bricks, int32_t capacity, int32_t C, int32_t pitch) {
    if (!votes || !table || n_bricks <= 0 || capacity <= 0 || C < 1 || C > 32) return false;
    return pitch >= C && (pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(votes) & 7) == 0;
}

// the host copy of a table: no slot at or past the capacity (and, when `no_missing`, none below zero)
bool slots_ok(const int32_t* table_host, int32_t n_bricks, int words, int32_t capacity, bool no_missing) {
    if (!table_host) return true;
    for (int32_t r = 0; r < n_bricks; ++r) {
        const int32_t slot = table_host[(size_t)r * words];
        if (slot >= capacity || (no_missing && slot < 0)) return false;
    }
    return true;
}

bool extract_ok(const OccdMapExtractArgs* a) {
    return a && pool_ok(a->votes, a->table, a->n_bricks, a->capacity, a->C, a->pitch) && a->min_obs >= 0 &&
           slots_ok(a->table_host, a->n_bricks, 4, a->capacity, false);
}

double pool_bytes(int32_t n_bricks, int32_t pitch) { return (double)n_bricks * kBrickVox * pitch * 2.0; }

// the weighted structs are the unweighted ones with one field renamed: the kernels take the unweighted struct either way
static_assert(sizeof(OccdMapWeightedArgs) == sizeof(OccdMapFrameArgs) &&
              offsetof(OccdMapWeightedArgs, weight) == offsetof(OccdMapFrameArgs, mask) &&
              offsetof(OccdMapWeightedArgs, label_bytes) == offsetof(OccdMapFrameArgs, label_bytes), "OccdMapWeightedArgs");
static_assert(sizeof(OccdMapSampleWeightedArgs) == sizeof(OccdMapSampleArgs) &&
              offsetof(OccdMapSampleWeightedArgs, own_weight) == offsetof(OccdMapSampleArgs, own_mask) &&
              offsetof(OccdMapSampleWeightedArgs, dq) == offsetof(OccdMapSampleArgs, dq), "OccdMapSampleWeightedArgs");

template <bool WEIGHTED>
int map_integrate(const OccdMapFrameArgs* a, void* stream) {
    if (!a || !a->labels || !pool_ok(a->votes, a->table, a->n_bricks, a->capacity, a->C, a->pitch)) return OCCD_EINVAL;
    if (WEIGHTED && !a->mask) return OCCD_EINVAL;
    if (a->X <= 0 || a->Y <= 0 || a->Z <= 0 || (int64_t)a->X * a->Y * a->Z > kMaxVox) return OCCD_EINVAL;
    if (a->label_bytes != 1 && a->label_bytes != 2) return OCCD_EINVAL;
    if (!slots_ok(a->table_host, a->n_bricks, 16, a->capacity, true)) return OCCD_EINVAL;
    const double frame = (double)a->X * a->Y * a->Z * (a->label_bytes + (a->mask ? 1 : 0));
    occd::ProfScope prof(WEIGHTED ? "map_integrate_weighted" : "map_integrate", (hipStream_t)stream, 0.0,
                         2.0 * pool_bytes(a->n_bricks, a->pitch) + frame);
    const dim3 grid((unsigned)a->n_bricks);
    if (a->label_bytes == 1) hipLaunchKernelGGL((map_integrate_kernel<1, WEIGHTED>), grid, dim3(kThreads), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL((map_integrate_kernel<2, WEIGHTED>), grid, dim3(kThreads), 0, (hipStream_t)stream, *a);
    return occd::check_launch();
}

template <bool WEIGHTED>
int map_sample(const OccdMapSampleArgs* a, void* stream) {
    if (!a || !a->cells || !a->labels || !a->n_obs || !pool_ok(a->votes, a->table, a->n_bricks, a->capacity, a->C, a->pitch))
        return OCCD_EINVAL;
    if (a->X <= 0 || a->Y <= 0 || a->Z <= 0 || (int64_t)a->X * a->Y * a->Z > kMaxVox) return OCCD_EINVAL;
    if (a->gx <= 0 || a->gy <= 0 || a->gz <= 0 || (int64_t)a->gx * a->gy * a->gz > kMaxCells) return OCCD_EINVAL;
    if ((a->flags & ~(OCCD_MAP_SAMPLE_EXCLUDE_SELF | OCCD_MAP_SAMPLE_KEEP_OWN)) != 0 || (a->flags != 0 && !a->own)) return OCCD_EINVAL;
    if (WEIGHTED && (a->flags & OCCD_MAP_SAMPLE_EXCLUDE_SELF) && !a->own_mask) return OCCD_EINVAL;
    if (a->min_obs < 0 || (a->label_bytes != 1 && a->label_bytes != 2)) return OCCD_EINVAL;
    if (!slots_ok(a->table_host, a->n_bricks, 16, a->capacity, false)) return OCCD_EINVAL;
    const double S = (double)a->X * a->Y * a->Z;
    // every voxel reads its vote row and writes 3 bytes; its own label, the mask and the directory come on top
    occd::ProfScope prof(WEIGHTED ? "map_sample_weighted" : "map_sample", (hipStream_t)stream, 0.0,
                         S * (a->pitch * 2.0 + 3.0 + (a->own ? a->label_bytes : 0)) + (double)a->gx * a->gy * a->gz * 4.0);
    const dim3 grid((unsigned)(((int64_t)a->X * a->Y * a->Z + kThreads - 1) / kThreads));
    if (a->label_bytes == 1) hipLaunchKernelGGL((map_sample_kernel<1, WEIGHTED>), grid, dim3(kThreads), 0, (hipStream_t)stream, *a);
    else hipLaunchKernelGGL((map_sample_kernel<2, WEIGHTED>), grid, dim3(kThreads), 0, (hipStream_t)stream, *a);
    return occd::check_launch();
}

}  // namespace

extern "C" int occd_map_integrate(const OccdMapFrameArgs* a, void* stream) { return map_integrate<false>(a, stream); }

extern "C" int occd_map_integrate_weighted(const OccdMapWeightedArgs* a, void* stream) {
    if (!a) return OCCD_EINVAL;
    OccdMapFrameArgs f;
    memcpy(&f, a, sizeof(f));                           // the same layout (asserted above), weight where mask is
    return map_integrate<true>(&f, stream);
}

extern "C" int occd_map_brick_labels(const OccdMapExtractArgs* a, void* stream) {
    if (!extract_ok(a) || !a->dense) return OCCD_EINVAL;
    occd::ProfScope prof("map_brick_labels", (hipStream_t)stream, 0.0, pool_bytes(a->n_bricks, a->pitch) + (double)a->n_bricks * kBrickVox);
    hipLaunchKernelGGL(map_brick_labels_kernel, dim3((unsigned)a->n_bricks), dim3(kThreads), 0, (hipStream_t)stream, *a);
    return occd::check_launch();
}

extern "C" int occd_map_count(const OccdMapExtractArgs* a, void* stream) {
    if (!extract_ok(a) || !a->counts) return OCCD_EINVAL;
    occd::ProfScope prof("map_count", (hipStream_t)stream, 0.0, pool_bytes(a->n_bricks, a->pitch));
    hipLaunchKernelGGL(map_scan_kernel<false>, dim3((unsigned)a->n_bricks), dim3(kThreads), 0, (hipStream_t)stream, *a);
    return occd::check_launch();
}

extern "C" int occd_map_extract(const OccdMapExtractArgs* a, void* stream) {
    if (!extract_ok(a) || !a->offsets || !a->coords || !a->labels || !a->n_obs || a->n_out <= 0) return OCCD_EINVAL;
    occd::ProfScope prof("map_extract", (hipStream_t)stream, 0.0, pool_bytes(a->n_bricks, a->pitch) + 15.0 * (double)a->n_out);
    hipLaunchKernelGGL(map_scan_kernel<true>, dim3((unsigned)a->n_bricks), dim3(kThreads), 0, (hipStream_t)stream, *a);
    return occd::check_launch();
}

extern "C" int occd_map_sample(const OccdMapSampleArgs* a, void* stream) { return map_sample<false>(a, stream); }

extern "C" int occd_map_sample_weighted(const OccdMapSampleWeightedArgs* a, void* stream) {
    if (!a) return OCCD_EINVAL;
    OccdMapSampleArgs f;
    memcpy(&f, a, sizeof(f));                           // the same layout (asserted above), own_weight where own_mask is
    return map_sample<true>(&f, stream);
}

extern "C" int occd_map_merge(const OccdMapMergeArgs* a, void* stream) {
    if (!a || !a->votes || !a->src || !a->table || a->n < 0 || a->capacity <= 0 || a->src_capacity <= 0) return OCCD_EINVAL;
    if (a->pitch < 4 || a->pitch > 32 || (a->pitch & 3) != 0) return OCCD_EINVAL;
    if (((reinterpret_cast<uintptr_t>(a->votes) | reinterpret_cast<uintptr_t>(a->src)) & 15) != 0) return OCCD_EINVAL;
    const int split = a->split != 0 ? a->split : (a->n < kMergeWhole ? kMergeSplit : 1);
    if (split != 1 && split != 2 && split != 4 && split != 8) return OCCD_EINVAL;
    if (a->table_host) {
        for (int32_t r = 0; r < a->n; ++r) {
            const int32_t slot = a->table_host[(size_t)r * 2], from = a->table_host[(size_t)r * 2 + 1];
            if (slot < 0 || slot >= a->capacity || from < 0 || from >= a->src_capacity) return OCCD_EINVAL;
        }
    }
    if (a->n == 0) return OCCD_OK;
    occd::ProfScope prof("map_merge", (hipStream_t)stream, 0.0, 3.0 * pool_bytes(a->n, a->pitch));
    const int pieces = kBrickVox / 8 * a->pitch / split;            // 512 * pitch / split: a multiple of 256 for every pitch
    hipLaunchKernelGGL(map_merge_kernel, dim3((unsigned)a->n, (unsigned)split), dim3(kThreads), 0, (hipStream_t)stream, *a, pieces);
    return occd::check_launch();
}
