// K38: stable segmented key/value radix sort, the repository's sort primitive (the Lovasz-softmax loss, csrc/lovasz.hip, is
// built on it).  LSD, kBits = 8 bits a pass, ping-pong buffers, three launches a pass:
//   hist_kernel     one workgroup per tile of kTile pairs: the tile's digit histogram (LDS atomics), written digit-major
//                   as hist[segment][digit][tile]
//   scan_kernel     one workgroup per segment: exclusive scan of that (digit, tile) table in place -- entry (d, t) becomes
//                   the position, within the segment, of the tile's first pair with digit d
//   scatter_kernel  one workgroup per tile: ranks the tile's pairs stably and moves them
// The stable rank inside a tile: wave w owns the contiguous quarter w of the tile and walks it 64 pairs at a time.  In a
// round the lanes that hold the same digit find each other with one __ballot per digit bit (64-bit masks); a lane's rank
// among them is the popcount of the mask below it, and the lowest of them adds the group's size to the wave's own digit
// counter in LDS.  After the rounds an exclusive sum over the four waves' counters and over the digits gives every pair
// its place in the tile ordered by digit; the tile is reordered through LDS, so that thread t then carries place t and a
// digit's run leaves as one stretch of consecutive addresses.
// No kernel waits for another workgroup (no look-back, no flags, no cooperative launch): the cross-tile prefixes come from
// the scan launch.  The grid depends on (segments, n) only; no allocation, no host read: capture-safe.  Integer arithmetic
// only: the output does not depend on the schedule.  Contract: include/occdepth_amd.h.
#include "common.h"

namespace {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int kBits = OCCD_SORT_RADIX_BITS;
constexpr int kDigits = 1 << kBits;              // 256 = the workgroup size of hist and scatter: thread d owns digit d
constexpr int kTile = OCCD_SORT_TILE;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kItems = kTile / kThreads;         // rounds of a wave over its quarter
constexpr int kScanThreads = 1024;
constexpr int kScanItems = 4;                    // consecutive entries per thread and iteration
static_assert(kDigits == kThreads, "thread d owns digit d");
static_assert(kTile % kThreads == 0 && (kTile / kWaves) % 64 == 0, "a wave walks its quarter in whole rounds");

struct SP {
    const u32* kin;
    const u32* vin;
    u32* kout;
    u32* vout;
    u32* hist;
    long n;
    u32 tiles;
    int shift;
    u32 mask;
};

__global__ void __launch_bounds__(kThreads) hist_kernel(const SP p) {
    __shared__ u32 h[kDigits];
    const u32 tile = blockIdx.x, seg = blockIdx.y;
    h[threadIdx.x] = 0;
    __syncthreads();
    const u32* k = p.kin + (size_t)seg * p.n;
    const long t0 = (long)tile * kTile;
#pragma unroll 4
    for (int j = 0; j < kItems; ++j) {
        const long i = t0 + j * kThreads + threadIdx.x;
        if (i < p.n) atomicAdd(&h[(k[i] >> p.shift) & p.mask], 1u);
    }
    __syncthreads();
    p.hist[((size_t)seg * kDigits + threadIdx.x) * p.tiles + tile] = h[threadIdx.x];
}

// exclusive scan of one segment's kDigits * tiles entries, in place; kScanThreads * kScanItems entries an iteration with a
// running carry
__global__ void __launch_bounds__(kScanThreads) scan_kernel(u32* hist, long len) {
    __shared__ u32 wsum[kScanThreads / 64];
    __shared__ u32 carry_sh;
    u32* h = hist + (size_t)blockIdx.x * len;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 carry = 0;
    for (long base = 0; base < len; base += (long)kScanThreads * kScanItems) {
        const long i0 = base + (long)threadIdx.x * kScanItems;
        u32 v[kScanItems];
        u32 sum = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            v[j] = i0 + j < len ? h[i0 + j] : 0u;
            sum += v[j];
        }
        u32 inc = sum;                             // inclusive scan over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        u32 before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (threadIdx.x == kScanThreads - 1) carry_sh = before + inc;
        u32 run = before + inc - sum;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            if (i0 + j < len) h[i0 + j] = run;
            run += v[j];
        }
        __syncthreads();
        carry = carry_sh;
    }
}

__global__ void __launch_bounds__(kThreads) scatter_kernel(const SP p) {
    __shared__ u32 cnt[kWaves][kDigits];           // per-wave digit counters, then the exclusive sums over the waves
    __shared__ u32 excl[kDigits];                  // first place of digit d in the tile ordered by digit
    __shared__ u32 gbase[kDigits];                 // position in the segment of the tile's first pair with digit d
    __shared__ u32 wtot[kWaves];
    __shared__ u32 sk[kTile], sv[kTile];
    const u32 tile = blockIdx.x, seg = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t sbase = (size_t)seg * p.n;
    const long t0 = (long)tile * kTile;
    const long left = p.n - t0;
    const int nvalid = left < kTile ? (int)left : kTile;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) cnt[w][tid] = 0;
    gbase[tid] = p.hist[((size_t)seg * kDigits + tid) * p.tiles + tile];
    __syncthreads();

    u32 key[kItems], val[kItems], rank[kItems];
    volatile u32* wc = cnt[wave];
    const u64 below = ((u64)1 << lane) - 1;
#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int loc = wave * (kTile / kWaves) + r * 64 + lane;      // place in the tile's input order
        const bool in = loc < nvalid;
        key[r] = in ? p.kin[sbase + t0 + loc] : 0u;
        val[r] = in ? p.vin[sbase + t0 + loc] : 0u;
        // a slot past the end takes the largest digit: it comes after every pair of the tile, in every order used here
        const u32 d = in ? (key[r] >> p.shift) & p.mask : p.mask;
        u64 peers = ~(u64)0;
#pragma unroll
        for (int b = 0; b < kBits; ++b) {
            const bool bit = (d >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const u32 pre = wc[d];
        __builtin_amdgcn_wave_barrier();
        if ((peers & below) == 0) wc[d] = pre + (u32)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        rank[r] = pre + (u32)__popcll(peers & below);
    }
    __syncthreads();

    // thread d: exclusive sums of digit d's counters over the waves, and of the digit totals over the digits
    {
        u32 run = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const u32 c = cnt[w][tid];
            cnt[w][tid] = run;
            run += c;
        }
        u32 inc = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u32 t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        u32 before = 0;
        for (int w = 0; w < wave; ++w) before += wtot[w];
        excl[tid] = before + inc - run;
    }
    __syncthreads();

#pragma unroll
    for (int r = 0; r < kItems; ++r) {
        const int loc = wave * (kTile / kWaves) + r * 64 + lane;
        const u32 d = loc < nvalid ? (key[r] >> p.shift) & p.mask : p.mask;
        const u32 pos = excl[d] + cnt[wave][d] + rank[r];             // < kTile: a permutation of the tile's slots
        sk[pos] = key[r];
        sv[pos] = val[r];
    }
    __syncthreads();

#pragma unroll
    for (int j = 0; j < kItems; ++j) {
        const int pos = j * kThreads + tid;
        if (pos < nvalid) {                                           // the slots past the end hold the last places
            const u32 k = sk[pos];
            const u32 d = (k >> p.shift) & p.mask;
            const size_t dst = sbase + gbase[d] + ((u32)pos - excl[d]);
            p.kout[dst] = k;
            p.vout[dst] = sv[pos];
        }
    }
}

}  // namespace

extern "C" int occd_sort_pairs_u32(const OccdSortArgs* a, void* stream) {
    if (!a || !a->keys || !a->vals || !a->keys_alt || !a->vals_alt || !a->hist) return OCCD_EINVAL;
    if (a->n < 1 || a->n > 0x7fffffffLL || a->segments < 1 || a->segments > 65535) return OCCD_EINVAL;
    if ((int64_t)a->segments * a->n >= ((int64_t)1 << 40)) return OCCD_EINVAL;
    if (a->begin_bit < 0 || a->begin_bit >= a->end_bit || a->end_bit > 32) return OCCD_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    SP p{};
    p.n = a->n;
    p.tiles = (u32)((a->n + kTile - 1) / kTile);
    p.hist = a->hist;
    const dim3 grid(p.tiles, (unsigned)a->segments);
    const double pairs = (double)a->segments * (double)a->n;
    int pass = 0;
    for (int bit = a->begin_bit; bit < a->end_bit; bit += kBits, ++pass) {
        const int width = a->end_bit - bit < kBits ? a->end_bit - bit : kBits;
        p.shift = bit;
        p.mask = (1u << width) - 1u;
        p.kin = pass & 1 ? a->keys_alt : a->keys;
        p.vin = pass & 1 ? a->vals_alt : a->vals;
        p.kout = pass & 1 ? a->keys : a->keys_alt;
        p.vout = pass & 1 ? a->vals : a->vals_alt;
        {
            occd::ProfScope prof("sort_hist", st, 0.0, pairs * 4.0);
            hipLaunchKernelGGL(hist_kernel, grid, dim3(kThreads), 0, st, p);
        }
        {
            occd::ProfScope prof("sort_scan", st, 0.0, (double)a->segments * kDigits * p.tiles * 8.0);
            hipLaunchKernelGGL(scan_kernel, dim3((unsigned)a->segments), dim3(kScanThreads), 0, st, a->hist,
                               (long)kDigits * p.tiles);
        }
        {
            occd::ProfScope prof("sort_scatter", st, 0.0, pairs * 16.0);
            hipLaunchKernelGGL(scatter_kernel, grid, dim3(kThreads), 0, st, p);
        }
        if (occd::check_launch() != OCCD_OK) return OCCD_ELAUNCH;
    }
    return OCCD_OK;
}
