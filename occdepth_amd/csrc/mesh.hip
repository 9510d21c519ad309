// K39: the surface of a brick volume as an indexed quad mesh (occd_mesh_count, occd_mesh_emit, occd_mesh_heads,
// occd_mesh_weld).  Contract: include/occdepth_amd.h.
//
// Count and emit are one kernel in two instantiations, shaped like map_scan_kernel of semantic_map.hip: a workgroup of 256
// threads takes one brick row, stages the brick (4096 bytes, one 16-byte load per thread) and the facing 16 x 16 planes
// of its six neighbour bricks (found through `cells`; 255 = unknown where there is none) in LDS, and walks the brick in 16
// passes of 256 voxels, thread tid = the voxel (pass, tid >> 4, tid & 15).  A voxel's six neighbour labels come from LDS,
// its face mask is six bits.  Faces are ranked in (voxel, face code) order without a loop over lanes: one ballot per face
// code, and mbcnt chained through the six masks counts every face of the lower lanes; the waves hand their totals over
// through LDS (two buffers, one barrier per pass).  A brick holds at most 12288 faces (the 3-D checkerboard); every
// position is offsets[row] + a sum of counts, so the output does not depend on the schedule.
//
// A row does not know its cell, so occd_mesh_count first inverts the directory into the workspace row_cell: a fill kernel
// and one thread per cell with an atomic minimum (the result of a minimum does not depend on the order; a well-formed
// directory names a row once).  A workgroup trusts row_cell only where cells[row_cell[row]] == row.
//
// Heads and weld are streams over the 4 F sorted corner references, one thread each.
#include <stddef.h>

#include "common.h"
#include "device.h"

namespace {

constexpr int kBrick = OCCD_MAP_BRICK;
constexpr int kBrickVox = kBrick * kBrick * kBrick;     // 4096
constexpr int kThreads = kBrick * kBrick;               // 256: one pass of the brick, one neighbour plane
constexpr int kWaves = kThreads / 64;
constexpr int32_t kNoCell = 0x7fffffff;
static_assert(kBrick == 16, "the thread layouts below are written for 16^3 bricks");

struct Geometry {
    int32_t n_cells;
    int32_t bx, by, bz;                                 // bits of a corner coordinate along each axis
};

__host__ __device__ inline int bit_length(uint32_t v) {
    int n = 0;
    while (v) { ++n; v >>= 1; }
    return n;
}

__global__ void __launch_bounds__(kThreads) mesh_fill_kernel(int32_t* p, int32_t n, int32_t value) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = value;
}

__global__ void __launch_bounds__(kThreads) mesh_rows_kernel(const int32_t* cells, int32_t n_cells, int32_t n_rows, int32_t* row_cell) {
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= n_cells) return;
    const int32_t r = cells[c];
    if (r >= 0 && r < n_rows) atomicMin(row_cell + r, (int32_t)c);
}

// WRITE = false: counts[row]; WRITE = true: the ordered write behind offsets[row]
template <bool WRITE>
__global__ void __launch_bounds__(kThreads) mesh_faces_kernel(const OccdMeshArgs a, const Geometry g) {
    __shared__ __attribute__((aligned(16))) uint8_t brick[kBrickVox];
    __shared__ uint8_t plane[6][kThreads];
    __shared__ int wave_n[2][kWaves];
    const int32_t row = (int32_t)blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t cell = a.row_cell[row];
    if (cell < 0 || cell >= g.n_cells || a.cells[cell] != row) {      // the whole workgroup: no cell points here
        if (!WRITE && tid == 0) a.counts[row] = 0;
        return;
    }
    int32_t cc[3];
    cc[2] = cell % a.gz;
    cc[1] = (cell / a.gz) % a.gy;
    cc[0] = cell / (a.gz * a.gy);
    const int32_t gdim[3] = {a.gx, a.gy, a.gz};
    reinterpret_cast<u32x4*>(brick)[tid] = reinterpret_cast<const u32x4*>(a.labels + (size_t)row * kBrickVox)[tid];
    const uint32_t p = (uint32_t)tid >> 4, q = (uint32_t)tid & 15u;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const int axis = d >> 1, side = d & 1;
        int32_t nc[3] = {cc[0], cc[1], cc[2]};
        nc[axis] += side ? 1 : -1;
        uint32_t lab = 255u;
        if (nc[axis] >= 0 && nc[axis] < gdim[axis]) {
            const int32_t r = a.cells[((size_t)nc[0] * (size_t)a.gy + (size_t)nc[1]) * (size_t)a.gz + (size_t)nc[2]];
            if (r >= 0 && r < a.n_rows) {
                const uint32_t at = side ? 0u : (uint32_t)(kBrick - 1);   // the neighbour's plane that touches this brick
                const uint32_t v = axis == 0 ? (at * kBrick + p) * kBrick + q
                                 : axis == 1 ? (p * kBrick + at) * kBrick + q
                                             : (p * kBrick + q) * kBrick + at;
                lab = a.labels[(size_t)r * kBrickVox + v];
            }
        }
        plane[d][tid] = (uint8_t)lab;
    }
    __syncthreads();

    const uint32_t j = p, l = q;
    const bool cap = a.cap_unknown != 0;
    int64_t out = WRITE ? a.offsets[row] : 0;
    int total = 0;
    for (int i = 0; i < kBrick; ++i) {
        const int v = i * kThreads + tid;
        const uint32_t lab = brick[v];
        uint32_t mask = 0;
        if (lab - 1u < 254u) {
            const uint32_t nb[6] = {i > 0 ? brick[v - kThreads] : plane[0][tid],
                                    i < kBrick - 1 ? brick[v + kThreads] : plane[1][tid],
                                    j > 0 ? brick[v - kBrick] : plane[2][i * kBrick + l],
                                    j < kBrick - 1 ? brick[v + kBrick] : plane[3][i * kBrick + l],
                                    l > 0 ? brick[v - 1] : plane[4][i * kBrick + j],
                                    l < kBrick - 1 ? brick[v + 1] : plane[5][i * kBrick + j]};
#pragma unroll
            for (int d = 0; d < 6; ++d) mask |= (uint32_t)(nb[d] == 0u || (cap && nb[d] == 255u)) << d;
        }
        uint32_t below = 0;                             // faces of the lower lanes of this wave
        int mine = 0;                                   // faces of this wave
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const unsigned long long m = __ballot((mask >> d) & 1u);
            below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, below));
            mine += __popcll(m);
        }
        if (lane == 0) wave_n[i & 1][wave] = mine;
        __syncthreads();                                // the other buffer is free: every wave passed the previous barrier
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const int n = wave_n[i & 1][w];
            all += n;
            before += w < wave ? n : 0;
        }
        if (WRITE && mask != 0u) {
            int64_t f = out + before + (int64_t)below;
            const uint32_t base[3] = {(uint32_t)cc[0] * kBrick + (uint32_t)i, (uint32_t)cc[1] * kBrick + j, (uint32_t)cc[2] * kBrick + l};
#pragma unroll
            for (int d = 0; d < 6; ++d) {
                if (!((mask >> d) & 1u)) continue;
                if (f >= 0 && f < a.n_faces) {          // offsets that do not belong to these counts write nothing
                    const int axis = d >> 1, side = d & 1;
                    const int second = side ? (axis + 1) % 3 : (axis + 2) % 3, last = side ? (axis + 2) % 3 : (axis + 1) % 3;
                    uint32_t lo[4], hi[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        uint32_t c[3] = {base[0], base[1], base[2]};
                        c[axis] += (uint32_t)side;
                        c[second] += (uint32_t)(k == 1 || k == 2);
                        c[last] += (uint32_t)(k == 2 || k == 3);
                        const uint64_t key = ((uint64_t)c[0] << (g.by + g.bz)) | ((uint64_t)c[1] << g.bz) | (uint64_t)c[2];
                        lo[k] = (uint32_t)key;
                        hi[k] = (uint32_t)(key >> 32);
                    }
                    const uint32_t r0 = (uint32_t)f * 4u;                     // 4 F < 2^31
                    a.face_label[f] = (uint8_t)lab;
                    a.face_dir[f] = (uint8_t)d;
                    reinterpret_cast<u32x4*>(a.keys_lo)[f] = u32x4{lo[0], lo[1], lo[2], lo[3]};
                    if (a.keys_hi != nullptr) reinterpret_cast<u32x4*>(a.keys_hi)[f] = u32x4{hi[0], hi[1], hi[2], hi[3]};
                    reinterpret_cast<u32x4*>(a.refs)[f] = u32x4{r0, r0 + 1u, r0 + 2u, r0 + 3u};
                }
                ++f;
            }
        }
        out += all;
        total += all;
    }
    if (!WRITE && tid == 0) a.counts[row] = total;
}

__global__ void __launch_bounds__(kThreads) mesh_heads_kernel(const OccdMeshArgs a, const int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    bool head = p == 0;
    if (!head) {
        head = a.keys_lo[p] != a.keys_lo[p - 1];
        if (a.keys_hi != nullptr) head = head || a.keys_hi[p] != a.keys_hi[p - 1];
    }
    a.marks[p] = head ? 1 : 0;
}

__global__ void __launch_bounds__(kThreads) mesh_weld_kernel(const OccdMeshArgs a, const Geometry g, const int64_t n) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const int32_t rank = a.ranks[p];
    const uint32_t ref = a.refs[p];
    if ((int64_t)ref >= n || rank < 1 || (int64_t)rank > a.n_vertices) return;
    a.quads[ref] = rank - 1;
    if (p == 0 || a.ranks[p - 1] != rank) {
        const uint64_t key = (uint64_t)a.keys_lo[p] | (a.keys_hi != nullptr ? (uint64_t)a.keys_hi[p] << 32 : 0ull);
        int32_t* out = a.vertices + (size_t)(rank - 1) * 3;
        out[0] = (int32_t)(key >> (g.by + g.bz));
        out[1] = (int32_t)((key >> g.bz) & ((1ull << g.by) - 1ull));
        out[2] = (int32_t)(key & ((1ull << g.bz) - 1ull));
    }
}

// the checks every stage shares; -> the directory size and the key layout
bool geometry_ok(const OccdMeshArgs* a, Geometry* g) {
    if (!a) return false;
    if (a->gx <= 0 || a->gy <= 0 || a->gz <= 0 || a->gx > OCCD_MESH_MAX_GRID || a->gy > OCCD_MESH_MAX_GRID || a->gz > OCCD_MESH_MAX_GRID)
        return false;
    const int64_t n_cells = (int64_t)a->gx * a->gy * a->gz;
    if (n_cells > OCCD_MESH_MAX_CELLS || a->n_rows <= 0) return false;
    g->n_cells = (int32_t)n_cells;
    g->bx = bit_length((uint32_t)a->gx * kBrick);
    g->by = bit_length((uint32_t)a->gy * kBrick);
    g->bz = bit_length((uint32_t)a->gz * kBrick);
    return g->bx + g->by + g->bz <= OCCD_MESH_MAX_KEY_BITS;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the volume: what count and emit read
bool volume_ok(const OccdMeshArgs* a, Geometry* g) {
    if (!geometry_ok(a, g) || !a->labels || !a->cells || !a->row_cell || !aligned16(a->labels)) return false;
    if (a->cells_host) {
        for (int32_t c = 0; c < g->n_cells; ++c)
            if (a->cells_host[c] >= a->n_rows) return false;
    }
    return true;
}

// the sorted corner references: what heads and weld read; -> 4 F
bool corners_ok(const OccdMeshArgs* a, Geometry* g, int64_t* n) {
    if (!geometry_ok(a, g) || !a->keys_lo || a->n_faces <= 0 || a->n_faces * 4 >= ((int64_t)1 << 31)) return false;
    if (g->bx + g->by + g->bz > 32 && !a->keys_hi) return false;
    *n = a->n_faces * 4;
    return true;
}

unsigned blocks(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int occd_mesh_count(const OccdMeshArgs* a, void* stream) {
    Geometry g;
    if (!volume_ok(a, &g) || !a->counts) return OCCD_EINVAL;
    occd::ProfScope prof("mesh_count", (hipStream_t)stream, 0.0, (double)a->n_rows * (kBrickVox + 6.0 * kThreads) + 4.0 * g.n_cells);
    hipLaunchKernelGGL(mesh_fill_kernel, dim3(blocks(a->n_rows)), dim3(kThreads), 0, (hipStream_t)stream, a->row_cell, a->n_rows, kNoCell);
    hipLaunchKernelGGL(mesh_rows_kernel, dim3(blocks(g.n_cells)), dim3(kThreads), 0, (hipStream_t)stream, a->cells, g.n_cells, a->n_rows,
                       a->row_cell);
    hipLaunchKernelGGL(mesh_faces_kernel<false>, dim3((unsigned)a->n_rows), dim3(kThreads), 0, (hipStream_t)stream, *a, g);
    return occd::check_launch();
}

extern "C" int occd_mesh_emit(const OccdMeshArgs* a, void* stream) {
    Geometry g;
    int64_t n;
    if (!volume_ok(a, &g) || !corners_ok(a, &g, &n)) return OCCD_EINVAL;
    if (!a->offsets || !a->face_label || !a->face_dir || !a->refs || !aligned16(a->keys_lo) || !aligned16(a->refs)) return OCCD_EINVAL;
    OccdMeshArgs k = *a;
    if (g.bx + g.by + g.bz <= 32) k.keys_hi = nullptr;                        // one word holds the key
    else if (!aligned16(k.keys_hi)) return OCCD_EINVAL;
    occd::ProfScope prof("mesh_emit", (hipStream_t)stream, 0.0,
                         (double)a->n_rows * (kBrickVox + 6.0 * kThreads) + (double)a->n_faces * (2.0 + (k.keys_hi ? 48.0 : 32.0)));
    hipLaunchKernelGGL(mesh_faces_kernel<true>, dim3((unsigned)a->n_rows), dim3(kThreads), 0, (hipStream_t)stream, k, g);
    return occd::check_launch();
}

extern "C" int occd_mesh_heads(const OccdMeshArgs* a, void* stream) {
    Geometry g;
    int64_t n;
    if (!corners_ok(a, &g, &n) || !a->marks) return OCCD_EINVAL;
    OccdMeshArgs k = *a;
    if (g.bx + g.by + g.bz <= 32) k.keys_hi = nullptr;
    occd::ProfScope prof("mesh_heads", (hipStream_t)stream, 0.0, (double)n * (k.keys_hi ? 12.0 : 8.0));
    hipLaunchKernelGGL(mesh_heads_kernel, dim3(blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, k, n);
    return occd::check_launch();
}

extern "C" int occd_mesh_weld(const OccdMeshArgs* a, void* stream) {
    Geometry g;
    int64_t n;
    if (!corners_ok(a, &g, &n) || !a->refs || !a->ranks || !a->quads || !a->vertices || a->n_vertices <= 0) return OCCD_EINVAL;
    OccdMeshArgs k = *a;
    if (g.bx + g.by + g.bz <= 32) k.keys_hi = nullptr;
    occd::ProfScope prof("mesh_weld", (hipStream_t)stream, 0.0, (double)n * (k.keys_hi ? 20.0 : 16.0) + 12.0 * (double)a->n_vertices);
    hipLaunchKernelGGL(mesh_weld_kernel, dim3(blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, k, g, n);
    return occd::check_launch();
}
