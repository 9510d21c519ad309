// K40: connected components of a label volume (occd_ccl_segments, occd_ccl_roots, occd_ccl_compact, occd_ccl_filter) and
// the exact overlap counts of two segment volumes (occd_ccl_pair_*).  Contract: include/occdepth_amd.h.
//
// Union-find with one invariant throughout: parent[v] <= v, a root is the smallest index of its tree, and a link goes
// from the larger root to the smaller through an atomic minimum.  Every value ever stored in parent[v] is a voxel of v's
// true component, so a reader that sees an old value sees an older ancestor, never a stranger.  The tile-local pass runs
// that union-find in LDS over a 16^3 tile (4096 int32 parents + 4096 label bytes + the tile's 256 stuff minima, 21 KiB)
// and leaves every voxel pointing at its tile-local root; the seam pass repeats it in global memory for the pairs that
// straddle tiles only.  Local and frame-linear indices are both lexicographic in (x, y, z), so the smallest local index
// of a tile-local component is its smallest frame-linear index too.
//
// Every data-dependent loop counts its steps against a bound made of the voxel count and, when it runs out, raises
// OCCD_CCL_STATUS_OVERRUN and falls through: no kernel spins, and none waits for another workgroup.
#include <stddef.h>

#include "common.h"
#include "device.h"

namespace {

constexpr int kTile = OCCD_CCL_TILE;
constexpr int kTileVox = kTile * kTile * kTile;         // 4096
constexpr int kThreads = 256;
constexpr int32_t kNone = 0x7fffffff;
static_assert(kTile == 16 && kThreads == kTile * kTile, "the thread layout below is one (y, z) plane of a 16^3 tile");

struct Masks {
    uint32_t things[8], stuff[8];
};

__device__ __forceinline__ bool in_mask(const uint32_t* m, uint32_t l) { return (m[l >> 5] >> (l & 31u)) & 1u; }

__device__ __forceinline__ void raise_status(int32_t* status, int32_t bit) { atomicOr(status, bit); }

// ---------------------------------------------------------------------------------------------- union-find in LDS
__device__ __forceinline__ int lds_find(volatile int* par, int a, bool& bad) {
    for (int it = 0; it <= kTileVox; ++it) {
        const int p = par[a];
        if (p == a) return a;
        a = p;
    }
    bad = true;
    return a;
}

__device__ __forceinline__ void lds_union(int* par, int a, int b, bool& bad) {
    for (int it = 0; it <= kTileVox; ++it) {
        a = lds_find(par, a, bad);
        b = lds_find(par, b, bad);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(par + hi, lo);
        if (old == hi) return;                          // hi was a root: this was the link
        a = old;                                        // hi had a parent already (old < hi): unite that with lo
        b = lo;
    }
    bad = true;
}

// ---------------------------------------------------------------------------------------------- union-find in memory
__device__ __forceinline__ int32_t load_parent(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of a, by agent-scope loads; a chain of more than one step is shortened (an ancestor is a legal parent)
__device__ __forceinline__ int32_t mem_find(int32_t* par, int32_t a, int32_t bound, bool& bad) {
    const int32_t from = a;
    int32_t steps = 0;
    for (;;) {
        const int32_t p = load_parent(par + a);
        if (p == a || p < 0) break;                     // p < 0: not a things voxel (only a corrupted workspace gets here)
        a = p;
        if (++steps > bound) {
            bad = true;
            break;
        }
    }
    if (steps > 1) atomicMin(par + from, a);
    return a;
}

__device__ __forceinline__ void mem_union(int32_t* par, int32_t a, int32_t b, int32_t bound, bool& bad) {
    for (int32_t it = 0; it <= bound; ++it) {
        a = mem_find(par, a, bound, bad);
        b = mem_find(par, b, bound, bad);
        if (a == b || bad) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicMin(par + hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
    bad = true;
}

// the neighbours that come before a voxel in (x, y, z) order: 3 under 6-connectivity (the first three), 13 under 26
__device__ __constant__ int8_t kBack[13][3] = {{-1, 0, 0},  {0, -1, 0},  {0, 0, -1},  {-1, -1, 0}, {-1, 1, 0},  {-1, 0, -1}, {-1, 0, 1},
                                               {0, -1, -1}, {0, -1, 1},  {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

// ---------------------------------------------------------------------------------------------- kernels
__global__ void __launch_bounds__(kThreads) ccl_fill_kernel(int32_t* p, int64_t n, int32_t value, int32_t* status) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = value;
    if (status != nullptr && i == 0) *status = 0;
}

// grid (tiles of a frame, B): the tile-local components
__global__ void __launch_bounds__(kThreads) ccl_tile_kernel(const OccdCclArgs a, const Masks m, const int32_t ty_n, const int32_t tz_n,
                                                            const int n_back) {
    __shared__ int par[kTileVox];
    __shared__ uint8_t lab[kTileVox];
    __shared__ int smin[256];
    const int tid = threadIdx.x, y = tid >> 4, z = tid & 15;
    const int32_t tile = (int32_t)blockIdx.x;
    const int32_t X0 = (tile / (ty_n * tz_n)) * kTile, Y0 = ((tile / tz_n) % ty_n) * kTile, Z0 = (tile % tz_n) * kTile;
    const size_t N = (size_t)a.X * a.Y * a.Z, base = (size_t)blockIdx.y * N;
    const bool col = Y0 + y < a.Y && Z0 + z < a.Z;                             // this thread's column lies in the frame
    const int32_t g0 = ((X0 * a.Y) + (Y0 + y)) * a.Z + (Z0 + z), gx = a.Y * a.Z;   // frame-linear index of (x, y, z): g0 + x gx
    smin[tid] = kNone;
    __syncthreads();
    for (int x = 0; x < kTile; ++x) {
        const int v = x * kThreads + tid;
        uint32_t l = 0;
        if (col && X0 + x < a.X) {
            l = a.labels[base + (size_t)(g0 + x * gx)];
            if (in_mask(m.stuff, l)) atomicMin(smin + l, g0 + x * gx);
            if (!in_mask(m.things, l)) l = 0;
            else if (l == 0) l = 256;                                          // things may name class 0: keep it apart from "none"
        }
        lab[v] = (uint8_t)(l == 256 ? 0 : l);
        par[v] = l != 0 ? v : -1;
    }
    __syncthreads();
    bool bad = false;
    for (int x = 0; x < kTile; ++x) {
        const int v = x * kThreads + tid;
        if (par[v] < 0) continue;                                              // -1 is never overwritten: no union touches it
        const uint32_t l = lab[v];
        for (int k = 0; k < n_back; ++k) {
            const int nx = x + kBack[k][0], ny = y + kBack[k][1], nz = z + kBack[k][2];
            if ((unsigned)nx >= (unsigned)kTile || (unsigned)ny >= (unsigned)kTile || (unsigned)nz >= (unsigned)kTile) continue;
            const int u = (nx * kTile + ny) * kTile + nz;
            if (((volatile int*)par)[u] < 0 || lab[u] != l) continue;
            lds_union(par, v, u, bad);
        }
    }
    __syncthreads();
    for (int x = 0; x < kTile; ++x) {
        const int v = x * kThreads + tid;
        if (!(col && X0 + x < a.X)) continue;
        int32_t out = -1;
        if (par[v] >= 0) {
            const int r = lds_find(par, v, bad);
            out = ((X0 + (r >> 8)) * a.Y + (Y0 + ((r >> 4) & 15))) * a.Z + (Z0 + (r & 15));
        }
        a.parent[base + (size_t)(g0 + x * gx)] = out;
    }
    if (smin[tid] != kNone) atomicMin(a.stuff_min + (size_t)blockIdx.y * 256 + tid, smin[tid]);
    if (bad) raise_status(a.status, OCCD_CCL_STATUS_OVERRUN);
}

// The stream kernels that lower a minimum or raise a count per class or segment take kChunk consecutive elements a
// workgroup and meet in LDS first: a frame's ground or facade would otherwise send 10^5 atomics to one address.
constexpr int kChunk = 16 * kThreads;                   // 4096

// OCCD_CCL_NO_TILE_PASS: every things voxel its own root; grid (chunks of a frame, B)
__global__ void __launch_bounds__(kThreads) ccl_init_kernel(const OccdCclArgs a, const Masks m, const int64_t N) {
    __shared__ int smin[256];
    const int tid = threadIdx.x;
    smin[tid] = kNone;
    __syncthreads();
    for (int it = 0; it < kChunk / kThreads; ++it) {
        const int64_t v = (int64_t)blockIdx.x * kChunk + it * kThreads + tid;
        if (v >= N) break;
        const size_t i = (size_t)blockIdx.y * (size_t)N + (size_t)v;
        const uint32_t l = a.labels[i];
        a.parent[i] = in_mask(m.things, l) ? (int32_t)v : -1;
        if (in_mask(m.stuff, l)) atomicMin(smin + l, (int32_t)v);
    }
    __syncthreads();
    if (smin[tid] != kNone) atomicMin(a.stuff_min + (size_t)blockIdx.y * 256 + tid, smin[tid]);
}

// grid (voxels of a frame, B): the pairs that straddle tiles (every pair when `tiled` is false)
__global__ void __launch_bounds__(kThreads) ccl_seam_kernel(const OccdCclArgs a, const Masks m, const int64_t N, const int n_back,
                                                            const bool tiled) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= N) return;
    const size_t base = (size_t)blockIdx.y * (size_t)N;
    const int32_t z = (int32_t)(v % a.Z), y = (int32_t)((v / a.Z) % a.Y), x = (int32_t)(v / ((int64_t)a.Z * a.Y));
    if (tiled && (x & 15) != 0 && (y & 15) != 0 && (y & 15) != 15 && (z & 15) != 0 && (z & 15) != 15) return;   // no neighbour leaves the tile
    const uint32_t l = a.labels[base + (size_t)v];
    if (!in_mask(m.things, l)) return;
    int32_t* par = a.parent + base;
    const int32_t bound = (int32_t)N;
    bool bad = false;
    for (int k = 0; k < n_back; ++k) {
        const int32_t nx = x + kBack[k][0], ny = y + kBack[k][1], nz = z + kBack[k][2];
        if (nx < 0 || ny < 0 || nz < 0 || ny >= a.Y || nz >= a.Z) continue;    // nx <= x < X
        if (tiled && (nx >> 4) == (x >> 4) && (ny >> 4) == (y >> 4) && (nz >> 4) == (z >> 4)) continue;
        const int32_t u = (nx * a.Y + ny) * a.Z + nz;
        if (a.labels[base + (size_t)u] != l) continue;
        mem_union(par, (int32_t)v, u, bound, bad);
    }
    if (bad) raise_status(a.status, OCCD_CCL_STATUS_OVERRUN);
}

// a launch of its own: parent is read only, after the launch boundary
__global__ void __launch_bounds__(kThreads) ccl_flatten_kernel(const OccdCclArgs a, const Masks m, const int64_t N) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= N) return;
    const size_t base = (size_t)blockIdx.y * (size_t)N, i = base + (size_t)v;
    const uint32_t l = a.labels[i];
    int32_t seg = 0;
    if (in_mask(m.things, l)) {
        const int32_t* par = a.parent + base;
        int32_t r = (int32_t)v, steps = 0;
        for (;;) {
            const int32_t p = par[r];
            if (p == r || p < 0) break;
            r = p;
            if (++steps > (int32_t)N) {
                raise_status(a.status, OCCD_CCL_STATUS_OVERRUN);
                break;
            }
        }
        seg = r + 1;
    } else if (in_mask(m.stuff, l)) {
        seg = a.stuff_min[(size_t)blockIdx.y * 256 + l] + 1;
    }
    a.seg[i] = seg;
}

// things segments by instance id: parent[b][id] = the smallest voxel index that carries id; grid (chunks of a frame, B)
__global__ void __launch_bounds__(kThreads) ccl_inst_min_kernel(const OccdCclArgs a, const Masks m, const int64_t N) {
    __shared__ int smin[256];
    const int tid = threadIdx.x;
    smin[tid] = kNone;
    __syncthreads();
    for (int it = 0; it < kChunk / kThreads; ++it) {
        const int64_t v = (int64_t)blockIdx.x * kChunk + it * kThreads + tid;
        if (v >= N) break;
        const size_t base = (size_t)blockIdx.y * (size_t)N, i = base + (size_t)v;
        const uint32_t l = a.labels[i];
        if (in_mask(m.things, l)) {
            const int32_t id = a.instances[i];
            if (id >= 1 && (int64_t)id < N) atomicMin(a.parent + base + (size_t)id, (int32_t)v);
        } else if (in_mask(m.stuff, l)) {
            atomicMin(smin + l, (int32_t)v);
        }
    }
    __syncthreads();
    if (smin[tid] != kNone) atomicMin(a.stuff_min + (size_t)blockIdx.y * 256 + tid, smin[tid]);
}

__global__ void __launch_bounds__(kThreads) ccl_inst_seg_kernel(const OccdCclArgs a, const Masks m, const int64_t N) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= N) return;
    const size_t base = (size_t)blockIdx.y * (size_t)N, i = base + (size_t)v;
    const uint32_t l = a.labels[i];
    int32_t seg = 0;
    if (in_mask(m.things, l)) {
        const int32_t id = a.instances[i];
        if (id >= 1 && (int64_t)id < N) {
            const int32_t first = a.parent[base + (size_t)id];
            if (first >= 0 && (int64_t)first < N) {
                if (a.labels[base + (size_t)first] != l) raise_status(a.status, OCCD_CCL_STATUS_INSTANCE);
                seg = first + 1;
            }
        }
    } else if (in_mask(m.stuff, l)) {
        seg = a.stuff_min[(size_t)blockIdx.y * 256 + l] + 1;
    }
    a.seg[i] = seg;
}

__global__ void __launch_bounds__(kThreads) ccl_roots_kernel(const int32_t* seg, int32_t* marks, const int64_t N, const int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= M) return;
    marks[i] = seg[i] == (int32_t)(i % N) + 1 ? 1 : 0;
}

// sizes[k] += 1 for every element with k >= 0, through a table of 256 (row, count) slots in LDS: a wave first folds its
// lanes by row (`todo` is wave-uniform: the loop does not diverge and clears at least one bit a round), the wave's first
// lane of a row claims the row's slot with a compare-and-swap or, where another row holds it, adds to memory at once; at
// the end every claimed slot adds its count to memory once.  Integer adds: the order does not matter.
struct RowTable {
    unsigned long long key[kThreads];
    int count[kThreads];
};
constexpr unsigned long long kNoRow = ~0ull;

__device__ __forceinline__ void table_add(RowTable& t, int32_t* sizes, int64_t k) {      // every lane of the wave calls it
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(k >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int64_t kl = __shfl(k, leader);
        const unsigned long long same = __ballot(k == kl) & todo;
        if (lane == leader) {
            const int n = (int)__popcll(same);
            const uint32_t slot = ((uint32_t)kl * 2654435761u) >> 24;
            const unsigned long long prev = atomicCAS(t.key + slot, kNoRow, (unsigned long long)kl);
            if (prev == kNoRow || prev == (unsigned long long)kl) atomicAdd(t.count + slot, n);
            else atomicAdd(sizes + kl, n);
        }
        todo &= ~same;
    }
}

__global__ void __launch_bounds__(kThreads) ccl_compact_kernel(const OccdCclArgs a, const int64_t N, const int64_t M) {
    __shared__ RowTable t;
    const int tid = threadIdx.x;
    t.key[tid] = kNoRow;
    t.count[tid] = 0;
    __syncthreads();
    for (int it = 0; it < kChunk / kThreads; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kChunk + it * kThreads + tid;
        int64_t k = -1;
        if (i < M) {
            const int64_t b = i / N;
            const int32_t s = a.seg[i];
            int32_t id = 0;
            if (s >= 1 && (int64_t)s <= N) id = a.ranks[b * N + (s - 1)];
            a.ids[i] = id;
            if (id >= 1 && a.seg_size != nullptr) {
                const int64_t row = a.offsets[b] + id - 1;
                if (row >= 0 && row < a.n_segments) {                          // ranks that do not belong to this seg write nothing
                    k = row;
                    if ((int64_t)s == i - b * N + 1) {
                        a.seg_class[row] = a.labels[i];
                        a.seg_index[row] = s - 1;
                    }
                }
            }
        }
        if (a.seg_size != nullptr) table_add(t, a.seg_size, k);
    }
    __syncthreads();
    if (a.seg_size != nullptr && t.key[tid] != kNoRow && t.count[tid] != 0) atomicAdd(a.seg_size + t.key[tid], t.count[tid]);
}

__global__ void __launch_bounds__(kThreads) ccl_sizes_kernel(const OccdCclArgs a, const Masks m, const int64_t N, const int64_t M) {
    __shared__ RowTable t;
    const int tid = threadIdx.x;
    t.key[tid] = kNoRow;
    t.count[tid] = 0;
    __syncthreads();
    for (int it = 0; it < kChunk / kThreads; ++it) {
        const int64_t i = (int64_t)blockIdx.x * kChunk + it * kThreads + tid;
        int64_t k = -1;
        if (i < M) {
            const int32_t s = a.seg[i];
            if (s >= 1 && (int64_t)s <= N && in_mask(m.things, a.labels[i])) k = (i / N) * N + (s - 1);
        }
        table_add(t, a.parent, k);
    }
    __syncthreads();
    if (t.key[tid] != kNoRow && t.count[tid] != 0) atomicAdd(a.parent + t.key[tid], t.count[tid]);
}

__global__ void __launch_bounds__(kThreads) ccl_filter_kernel(const OccdCclArgs a, const Masks m, const int64_t N, const int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= M) return;
    uint32_t l = a.labels[i];
    const int32_t s = a.seg[i];
    if (s >= 1 && (int64_t)s <= N && in_mask(m.things, l) && a.parent[(i / N) * N + (s - 1)] < a.min_voxels) l = 0;
    a.out[i] = (uint8_t)l;
}

// ---------------------------------------------------------------------------------------------- overlaps
__device__ __forceinline__ bool pair_marked(const OccdCclPairArgs& a, int64_t i) {
    if (a.target[i] == 255 || (a.mask != nullptr && a.mask[i] == 0)) return false;
    return (a.g_ids[i] | a.p_ids[i]) != 0;
}

__global__ void __launch_bounds__(kThreads) pair_marks_kernel(const OccdCclPairArgs a, const int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < M) a.marks[i] = pair_marked(a, i) ? 1 : 0;
}

__global__ void __launch_bounds__(kThreads) pair_emit_kernel(const OccdCclPairArgs a, const int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= M || !pair_marked(a, i)) return;
    const int64_t q = (int64_t)a.pos[i] - 1;
    if (q < 0 || q >= a.n_pairs) return;                // a scan that does not belong to these marks writes nothing
    const int64_t b = i / a.n;
    const int32_t gi = a.g_ids[i], pi = a.p_ids[i];
    const uint32_t g = gi > 0 ? (uint32_t)(a.g_offsets[b] + gi) : 0u, p = pi > 0 ? (uint32_t)(a.p_offsets[b] + pi) : 0u;
    if (a.keys_hi != nullptr) {
        a.keys_lo[q] = p;
        a.keys_hi[q] = g;
    } else {
        a.keys_lo[q] = (g << a.p_bits) | p;
    }
    a.refs[q] = (uint32_t)q;
}

__global__ void __launch_bounds__(kThreads) pair_heads_kernel(const OccdCclPairArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= a.n_pairs) return;
    bool head = q == 0;
    if (!head) {
        head = a.keys_lo[q] != a.keys_lo[q - 1];
        if (a.keys_hi != nullptr) head = head || a.keys_hi[q] != a.keys_hi[q - 1];
    }
    a.marks[q] = head ? 1 : 0;
}

__global__ void __launch_bounds__(kThreads) pair_rows_kernel(const OccdCclPairArgs a) {
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= a.n_pairs) return;
    const int32_t r = a.ranks[q];
    if (r < 1 || (int64_t)r > a.n_rows || (q > 0 && a.ranks[q - 1] == r)) return;
    const uint32_t lo = a.keys_lo[q];
    a.row_start[r - 1] = (int32_t)q;
    if (a.keys_hi != nullptr) {
        a.row_g[r - 1] = (int32_t)a.keys_hi[q];
        a.row_p[r - 1] = (int32_t)lo;
    } else {
        a.row_g[r - 1] = a.p_bits >= 32 ? 0 : (int32_t)(lo >> a.p_bits);
        a.row_p[r - 1] = (int32_t)(a.p_bits >= 32 ? lo : lo & ((1u << a.p_bits) - 1u));
    }
}

__global__ void __launch_bounds__(kThreads) pair_lengths_kernel(const OccdCclPairArgs a) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= a.n_rows) return;
    const int64_t end = r + 1 < a.n_rows ? (int64_t)a.row_start[r + 1] : a.n_pairs;
    a.row_n[r] = (int32_t)(end - a.row_start[r]);
}

// ---------------------------------------------------------------------------------------------- host side
unsigned blocks(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// the volume every stage shares -> N and M = B N
bool volume_ok(const OccdCclArgs* a, int64_t* N, int64_t* M) {
    if (!a || a->batch < 1 || a->batch > 65535 || a->X < 1 || a->Y < 1 || a->Z < 1) return false;
    const int64_t xy = (int64_t)a->X * a->Y;
    if (xy >= ((int64_t)1 << 31)) return false;
    *N = xy * a->Z;
    if (*N >= ((int64_t)1 << 31) - 1) return false;
    *M = *N * a->batch;
    return *M < ((int64_t)1 << 40);
}

bool masks_ok(const OccdCclArgs* a, Masks* m) {
    for (int w = 0; w < 8; ++w) {
        if (a->things[w] & a->stuff[w]) return false;
        m->things[w] = a->things[w];
        m->stuff[w] = a->stuff[w];
    }
    return true;
}

bool pairs_ok(const OccdCclPairArgs* a, int64_t* M) {
    if (!a || a->batch < 1 || a->n < 1 || a->n >= ((int64_t)1 << 31)) return false;
    *M = a->n * a->batch;
    if (*M >= ((int64_t)1 << 31)) return false;
    return a->p_bits >= 1 && a->p_bits <= 32 && (a->keys_hi != nullptr || a->p_bits <= 31);
}

}  // namespace

extern "C" int occd_ccl_segments(const OccdCclArgs* a, void* stream) {
    int64_t N, M;
    Masks m;
    if (!volume_ok(a, &N, &M) || !masks_ok(a, &m)) return OCCD_EINVAL;
    if (!a->labels || !a->parent || !a->stuff_min || !a->status || !a->seg) return OCCD_EINVAL;
    if (a->connectivity != 6 && a->connectivity != 26) return OCCD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int n_back = a->connectivity == 6 ? 3 : 13;
    const dim3 vox(blocks(N), (unsigned)a->batch), chunks((unsigned)((N + kChunk - 1) / kChunk), (unsigned)a->batch);
    if (a->instances != nullptr) {
        occd::ProfScope prof("ccl_instances", s, 0.0, (double)M * 22.0);
        hipLaunchKernelGGL(ccl_fill_kernel, dim3(blocks(256 * (int64_t)a->batch)), dim3(kThreads), 0, s, a->stuff_min, 256 * (int64_t)a->batch,
                           kNone, a->status);
        hipLaunchKernelGGL(ccl_fill_kernel, dim3(blocks(M)), dim3(kThreads), 0, s, a->parent, M, kNone, (int32_t*)nullptr);
        hipLaunchKernelGGL(ccl_inst_min_kernel, chunks, dim3(kThreads), 0, s, *a, m, N);
        hipLaunchKernelGGL(ccl_inst_seg_kernel, vox, dim3(kThreads), 0, s, *a, m, N);
        return occd::check_launch();
    }
    const bool tiled = !(a->flags & OCCD_CCL_NO_TILE_PASS);
    {                                                   // one profile row per stage: tools/bench_ccl.py reads them
        occd::ProfScope prof(tiled ? "ccl_tile" : "ccl_init", s, 0.0, (double)M * 5.0);
        hipLaunchKernelGGL(ccl_fill_kernel, dim3(blocks(256 * (int64_t)a->batch)), dim3(kThreads), 0, s, a->stuff_min, 256 * (int64_t)a->batch,
                           kNone, a->status);
        if (tiled) {
            const int32_t tx = (a->X + kTile - 1) / kTile, ty = (a->Y + kTile - 1) / kTile, tz = (a->Z + kTile - 1) / kTile;
            hipLaunchKernelGGL(ccl_tile_kernel, dim3((unsigned)(tx * ty * tz), (unsigned)a->batch), dim3(kThreads), 0, s, *a, m, ty, tz, n_back);
        } else {
            hipLaunchKernelGGL(ccl_init_kernel, chunks, dim3(kThreads), 0, s, *a, m, N);
        }
    }
    {
        occd::ProfScope prof(tiled ? "ccl_seam" : "ccl_seam_all", s, 0.0, (double)M);
        hipLaunchKernelGGL(ccl_seam_kernel, vox, dim3(kThreads), 0, s, *a, m, N, n_back, tiled);
    }
    {
        occd::ProfScope prof("ccl_flatten", s, 0.0, (double)M * 9.0);
        hipLaunchKernelGGL(ccl_flatten_kernel, vox, dim3(kThreads), 0, s, *a, m, N);
    }
    return occd::check_launch();
}

extern "C" int occd_ccl_roots(const OccdCclArgs* a, void* stream) {
    int64_t N, M;
    if (!volume_ok(a, &N, &M) || !a->seg || !a->marks) return OCCD_EINVAL;
    occd::ProfScope prof("ccl_roots", (hipStream_t)stream, 0.0, (double)M * 8.0);
    hipLaunchKernelGGL(ccl_roots_kernel, dim3(blocks(M)), dim3(kThreads), 0, (hipStream_t)stream, a->seg, a->marks, N, M);
    return occd::check_launch();
}

extern "C" int occd_ccl_compact(const OccdCclArgs* a, void* stream) {
    int64_t N, M;
    if (!volume_ok(a, &N, &M) || !a->seg || !a->ranks || !a->offsets || !a->ids || a->n_segments < 0) return OCCD_EINVAL;
    if (a->n_segments > 0 && (!a->labels || !a->seg_class || !a->seg_size || !a->seg_index)) return OCCD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    OccdCclArgs k = *a;
    if (k.n_segments == 0) k.seg_size = nullptr;
    occd::ProfScope prof("ccl_compact", s, 0.0, (double)M * 12.0 + (double)a->n_segments * 13.0);
    if (k.seg_size != nullptr)
        hipLaunchKernelGGL(ccl_fill_kernel, dim3(blocks(k.n_segments)), dim3(kThreads), 0, s, k.seg_size, k.n_segments, 0, (int32_t*)nullptr);
    hipLaunchKernelGGL(ccl_compact_kernel, dim3((unsigned)((M + kChunk - 1) / kChunk)), dim3(kThreads), 0, s, k, N, M);
    return occd::check_launch();
}

extern "C" int occd_ccl_filter(const OccdCclArgs* a, void* stream) {
    int64_t N, M;
    Masks m;
    if (!volume_ok(a, &N, &M) || !masks_ok(a, &m)) return OCCD_EINVAL;
    if (!a->labels || !a->seg || !a->parent || !a->out || a->min_voxels < 1) return OCCD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    occd::ProfScope prof("ccl_filter", s, 0.0, (double)M * 22.0);
    hipLaunchKernelGGL(ccl_fill_kernel, dim3(blocks(M)), dim3(kThreads), 0, s, a->parent, M, 0, (int32_t*)nullptr);
    hipLaunchKernelGGL(ccl_sizes_kernel, dim3((unsigned)((M + kChunk - 1) / kChunk)), dim3(kThreads), 0, s, *a, m, N, M);
    hipLaunchKernelGGL(ccl_filter_kernel, dim3(blocks(M)), dim3(kThreads), 0, s, *a, m, N, M);
    return occd::check_launch();
}

extern "C" int occd_ccl_pair_marks(const OccdCclPairArgs* a, void* stream) {
    int64_t M;
    if (!pairs_ok(a, &M) || !a->g_ids || !a->p_ids || !a->target || !a->marks) return OCCD_EINVAL;
    occd::ProfScope prof("ccl_pair_marks", (hipStream_t)stream, 0.0, (double)M * 13.0);
    hipLaunchKernelGGL(pair_marks_kernel, dim3(blocks(M)), dim3(kThreads), 0, (hipStream_t)stream, *a, M);
    return occd::check_launch();
}

extern "C" int occd_ccl_pair_emit(const OccdCclPairArgs* a, void* stream) {
    int64_t M;
    if (!pairs_ok(a, &M) || !a->g_ids || !a->p_ids || !a->target || !a->pos || !a->g_offsets || !a->p_offsets) return OCCD_EINVAL;
    if (!a->keys_lo || !a->refs || a->n_pairs < 1 || a->n_pairs > M) return OCCD_EINVAL;
    occd::ProfScope prof("ccl_pair_emit", (hipStream_t)stream, 0.0, (double)M * 14.0 + (double)a->n_pairs * 12.0);
    hipLaunchKernelGGL(pair_emit_kernel, dim3(blocks(M)), dim3(kThreads), 0, (hipStream_t)stream, *a, M);
    return occd::check_launch();
}

extern "C" int occd_ccl_pair_heads(const OccdCclPairArgs* a, void* stream) {
    int64_t M;
    if (!pairs_ok(a, &M) || !a->keys_lo || !a->marks || a->n_pairs < 1 || a->n_pairs > M) return OCCD_EINVAL;
    occd::ProfScope prof("ccl_pair_heads", (hipStream_t)stream, 0.0, (double)a->n_pairs * 12.0);
    hipLaunchKernelGGL(pair_heads_kernel, dim3(blocks(a->n_pairs)), dim3(kThreads), 0, (hipStream_t)stream, *a);
    return occd::check_launch();
}

extern "C" int occd_ccl_pair_rows(const OccdCclPairArgs* a, void* stream) {
    int64_t M;
    if (!pairs_ok(a, &M) || !a->keys_lo || !a->ranks || !a->row_start || !a->row_g || !a->row_p || !a->row_n) return OCCD_EINVAL;
    if (a->n_pairs < 1 || a->n_pairs > M || a->n_rows < 1 || a->n_rows > a->n_pairs) return OCCD_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    occd::ProfScope prof("ccl_pair_rows", s, 0.0, (double)a->n_pairs * 12.0 + (double)a->n_rows * 20.0);
    hipLaunchKernelGGL(pair_rows_kernel, dim3(blocks(a->n_pairs)), dim3(kThreads), 0, s, *a);
    hipLaunchKernelGGL(pair_lengths_kernel, dim3(blocks(a->n_rows)), dim3(kThreads), 0, s, *a);
    return occd::check_launch();
}
