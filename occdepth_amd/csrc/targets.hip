// Training targets of the SemanticKITTI dataloader on the GPU (include/occdepth_amd.h, "Training targets"):
//
//   frustum_targets_kernel   compute_local_frustums   occdepth/data/utils/helpers.py:183-260 (dataset "kitti")
//   downsample_label_kernel  _downsample_label        occdepth/data/NYU/preprocess.py:102-143
//   cp_mega_kernel           compute_CP_mega_matrix   occdepth/data/utils/helpers.py:6-91
//   kitti_labels_kernel      the label decode of       occdepth/data/semantic_kitti/preprocess.py:76-84 (io_data.py:10-22,
//                            the preprocessing pass    122-134,175-195) and the `.occluded` volume of kitti_dataset.py:312-313
//
// All three are bit-exact: projection through occd::project_one (the integers of the dataloader's vox2pix), frustum
// bounds compared in float64 as numpy does, integer counters (LDS histograms flushed with integer atomics: deterministic).
// Capture-safe: calibration is read from device memory, counters are zeroed by a fill kernel (not hipMemsetAsync).
#include "common.h"
#include "project.h"

namespace {

constexpr int kMaxFrustum = 16;        // frustum_size s <= 16
constexpr int kMaxBins = 4096;         // F * n_classes LDS counters
constexpr int kVoxPerThread = 16;      // one 16-byte mask store per lane and frustum
constexpr int kVoxPerBlock = 256 * kVoxPerThread;
constexpr uint32_t kNone = 0xFFFFu;    // "in no frustum" (16-bit frustum code per view)

struct FrustumP {
    const double* cam_E;
    const double* cam_k;
    const uint8_t* target;
    uint8_t* masks;
    uint32_t* counts;                  // the float32 dists buffer, as counters until frustum_counts_to_float
    double sx[kMaxFrustum + 1];        // (i * 1.0 / s) * W, helpers.py:208,214-215
    double sy[kMaxFrustum + 1];        // (j * 1.0 / s) * H
    double vox_size;
    float origin[3];
    int X, Y, Z, N, img_w, img_h, s, F, C;
    int vec;                           // N % 16 == 0: 16-byte mask stores
};

__global__ void __launch_bounds__(256) frustum_zero_kernel(uint32_t* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

__global__ void __launch_bounds__(256) frustum_counts_to_float(uint32_t* p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const uint32_t c = p[i];
        reinterpret_cast<float*>(p)[i] = (float)c;
    }
}

// tile of an integer pixel coordinate: the i with lo[i] <= pix < lo[i + 1] (float64 compares), or -1
__device__ __forceinline__ int tile_of(long pix, const double* lo, int s) {
    const double v = (double)pix;                         // exact: |pix| <= 1e9
    int t = -1;
#pragma unroll
    for (int i = 0; i < kMaxFrustum; ++i)
        if (i < s && v >= lo[i] && v < lo[i + 1]) t = i;
    return t;
}

// A workgroup owns 4096 consecutive voxels of one sample.  Phase A: each lane projects 16 of them (stride 256, coalesced
// target loads) through the V views, keeps one 32-bit code per voxel in LDS (frustum of view 0 | frustum of view 1 << 16,
// 0xFFFF = none or unlabelled) and counts (frustum, class) in an LDS histogram.  Phase B: each lane turns 16 consecutive
// codes into one 16-byte mask word per frustum.  The histogram is flushed with one integer atomic per non-zero bin.
template <int V>
__global__ void __launch_bounds__(256) frustum_targets_kernel(const FrustumP p) {
    __shared__ uint32_t s_code[kVoxPerBlock];
    __shared__ uint32_t s_hist[kMaxBins];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int bins = p.F * p.C;
    for (int i = tid; i < bins; i += 256) s_hist[i] = 0u;

    double E[V][16], fx[V], fy[V], cx[V], cy[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const double* e = p.cam_E + ((size_t)b * V + v) * 16;
        const double* k = p.cam_k + ((size_t)b * V + v) * 9;
#pragma unroll
        for (int j = 0; j < 16; ++j) E[v][j] = e[j];
        fx[v] = (double)(float)k[0];
        fy[v] = (double)(float)k[4];
        cx[v] = (double)(float)k[2];
        cy[v] = (double)(float)k[5];
    }
    __syncthreads();

    const long base = (long)blockIdx.x * kVoxPerBlock;
    const uint8_t* tgt = p.target + (size_t)b * p.N;
    // ---- phase A
    for (int k = 0; k < kVoxPerThread; ++k) {
        const int loc = k * 256 + tid;
        const long n = base + loc;
        uint32_t code = kNone | (kNone << 16);
        if (n < p.N) {
            const int t = tgt[n];
            if (t != 255) {
                const uint32_t n32 = (uint32_t)n;
                const uint32_t yz = (uint32_t)p.Y * (uint32_t)p.Z;
                const int ix = (int)(n32 / yz);
                const uint32_t r = n32 - (uint32_t)ix * yz;
                const int iy = (int)(r / (uint32_t)p.Z), iz = (int)(r - (uint32_t)iy * (uint32_t)p.Z);
                uint32_t f[2] = {kNone, kNone};
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    long px, py;
                    double camz;
                    occd::project_one(E[v], fx[v], fy[v], cx[v], cy[v], p.vox_size, p.origin, ix, iy, iz, p.img_w,
                                      p.img_h, px, py, camz);
                    const int ti = tile_of(px, p.sx, p.s), tj = tile_of(py, p.sy, p.s);
                    if (camz > 0.0 && ti >= 0 && tj >= 0) f[v] = (uint32_t)(tj * p.s + ti);
                }
                code = f[0] | (f[1] << 16);
                if (t < p.C) {
                    if (f[0] != kNone) atomicAdd(&s_hist[f[0] * p.C + t], 1u);
                    if (V == 2 && f[1] != kNone && f[1] != f[0]) atomicAdd(&s_hist[f[1] * p.C + t], 1u);
                }
            }
        }
        s_code[loc] = code;
    }
    __syncthreads();

    // ---- phase B: lane -> voxels [base + 16 tid, base + 16 tid + 16)
    uint32_t c[kVoxPerThread];
#pragma unroll
    for (int k = 0; k < kVoxPerThread; ++k) c[k] = s_code[tid * kVoxPerThread + k];
    const long n0 = base + (long)tid * kVoxPerThread;
    if (n0 < p.N) {
        uint8_t* out = p.masks + (size_t)b * p.F * p.N + n0;
        const bool full = p.vec && n0 + kVoxPerThread <= p.N;
        for (int f = 0; f < p.F; ++f) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < kVoxPerThread; ++k) {
                const bool in = (c[k] & 0xFFFFu) == (uint32_t)f || (c[k] >> 16) == (uint32_t)f;
                w[k >> 2] |= (in ? 1u : 0u) << ((k & 3) * 8);
            }
            uint8_t* row = out + (size_t)f * p.N;
            if (full) {
                *reinterpret_cast<uint4*>(row) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll
                for (int k = 0; k < kVoxPerThread; ++k)
                    if (n0 + k < p.N) row[k] = (uint8_t)((w[k >> 2] >> ((k & 3) * 8)) & 0xFFu);
            }
        }
    }

    uint32_t* cnt = p.counts + (size_t)b * bins;
    for (int i = tid; i < bins; i += 256) {
        const uint32_t h = s_hist[i];
        if (h) atomicAdd(&cnt[i], h);
    }
}

// One wavefront per coarse voxel: LDS histogram of the ds^3 labels, then a wave max over (count, -label) keys.
__global__ void __launch_bounds__(256) downsample_label_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                               int X, int Y, int Z, int ds, long n_out, double empty_t) {
    __shared__ uint32_t s_hist[4][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long o = (long)blockIdx.x * 4 + w;           // flat (b, x, y, z) of the output
    uint32_t* h = s_hist[w];
#pragma unroll
    for (int i = 0; i < 4; ++i) h[lane + 64 * i] = 0u;
    __syncthreads();
    const int Xs = X / ds, Ys = Y / ds, Zs = Z / ds;
    if (o < n_out) {
        const int zs = (int)(o % Zs);
        long t = o / Zs;
        const int ys = (int)(t % Ys);
        t /= Ys;
        const int xs = (int)(t % Xs);
        const long b = t / Xs;
        const uint8_t* src = in + (size_t)b * X * Y * Z;
        const int vol = ds * ds * ds;
        for (int i = lane; i < vol; i += 64) {
            const int dz = i % ds, dy = (i / ds) % ds, dx = i / (ds * ds);
            const int lab = src[((size_t)(xs * ds + dx) * Y + (ys * ds + dy)) * Z + (zs * ds + dz)];
            atomicAdd(&h[lab], 1u);
        }
    }
    __syncthreads();
    if (o >= n_out) return;
    // key = count << 8 | (255 - label) over labels 1..254: the largest key is np.argmax(np.bincount(...))
    uint32_t best = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int lab = lane + 64 * i;
        if (lab >= 1 && lab <= 254) {
            const uint32_t key = (h[lab] << 8) | (uint32_t)(255 - lab);
            if (h[lab] && key > best) best = key;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)best, m, 64);
        best = other > best ? other : best;
    }
    if (lane == 0) {
        const uint32_t c0 = h[0], c255 = h[255];
        uint8_t v;
        if ((double)(c0 + c255) > empty_t) v = c0 > c255 ? 0 : 255;
        else v = (uint8_t)(255u - (best & 0xFFu));
        out[o] = v;
    }
}

// 256-bit set of the non-255 child labels of every mega voxel (built per workgroup in LDS), then lanes along M: one lane
// writes 16 consecutive mega-voxel bytes of one row for each of the R relation planes.
constexpr int kMegaTile = 512;        // mega voxels per workgroup (32 lanes x 16)
constexpr int kRowsPerBlock = 16;

__global__ void __launch_bounds__(256) cp_mega_kernel(const uint8_t* __restrict__ coarse, uint8_t* __restrict__ out,
                                                      int X, int Y, int Z, long N, long M, int binary) {
    __shared__ uint64_t s_set[kMegaTile][4];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const long m_base = (long)blockIdx.y * kMegaTile;
    const uint8_t* lab = coarse + (size_t)b * N;
    const int Ym = Y / 2, Zm = Z / 2;
    for (int i = tid; i < kMegaTile; i += 256) {
        uint64_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        const long m = m_base + i;
        if (m < M) {
            const int zz = (int)(m % Zm);
            const long t = m / Zm;
            const int yy = (int)(t % Ym), xx = (int)(t / Ym);
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int x = 2 * xx + (d & 1), y = 2 * yy + ((d >> 1) & 1), z = 2 * zz + (d >> 2);
                const int l = lab[((size_t)x * Y + y) * Z + z];
                if (l == 255) continue;
                const uint64_t bit = 1ull << (l & 63);
                const int q = l >> 6;
                s0 |= q == 0 ? bit : 0ull;
                s1 |= q == 1 ? bit : 0ull;
                s2 |= q == 2 ? bit : 0ull;
                s3 |= q == 3 ? bit : 0ull;
            }
        }
        s_set[i][0] = s0;
        s_set[i][1] = s1;
        s_set[i][2] = s2;
        s_set[i][3] = s3;
    }
    __syncthreads();

    const int R = binary ? 2 : 4;
    const int mc = tid & 31, ry = tid >> 5;                 // 32 lanes x 16 bytes along M, 8 rows per pass
    const long m0 = m_base + (long)mc * 16;
    if (m0 >= M) return;
    const bool full = (M & 15) == 0 && m0 + 16 <= M;
    for (int rr = ry; rr < kRowsPerBlock; rr += 8) {
        const long n = (long)blockIdx.x * kRowsPerBlock + rr;
        if (n >= N) break;
        const int row = lab[n];
        uint32_t w[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) w[r][q] = 0u;
        if (row != 255) {
            const int rq = row >> 6;
            const uint64_t rbit = 1ull << (row & 63);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int i = mc * 16 + k;
                const uint64_t a0 = s_set[i][0], a1 = s_set[i][1], a2 = s_set[i][2], a3 = s_set[i][3];
                const uint64_t mine = rq == 0 ? a0 : rq == 1 ? a1 : rq == 2 ? a2 : a3;
                const bool has_row = (mine & rbit) != 0;                               // row label among the children
                const bool has_zero = (a0 & 1ull) != 0;                                // label 0 among the children
                const uint64_t o0 = a0 & ~(rq == 0 ? rbit : 0ull), o1 = a1 & ~(rq == 1 ? rbit : 0ull);
                const uint64_t o2 = a2 & ~(rq == 2 ? rbit : 0ull), o3 = a3 & ~(rq == 3 ? rbit : 0ull);
                const bool has_other = (o0 | o1 | o2 | o3) != 0;                       // some child label != row
                const bool has_other_nz = ((o0 & ~1ull) | o1 | o2 | o3) != 0;          // ... != row and != 0
                bool v[4];
                if (binary) {
                    v[0] = has_other;                                   // diff
                    v[1] = has_row;                                     // same
                    v[2] = v[3] = false;
                } else {
                    v[0] = row != 0 && has_row;                         // non non same
                    v[1] = row != 0 && has_other_nz;                    // non non diff
                    v[2] = row == 0 && has_zero;                        // empty empty
                    v[3] = row == 0 ? has_other_nz : has_zero;          // nonempty empty
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r][k >> 2] |= (v[r] ? 1u : 0u) << ((k & 3) * 8);
            }
        }
        for (int r = 0; r < R; ++r) {
            uint8_t* dst = out + (((size_t)b * R + r) * N + n) * M + m0;
            if (full) {
                *reinterpret_cast<uint4*>(dst) = make_uint4(w[r][0], w[r][1], w[r][2], w[r][3]);
            } else {
                for (int k = 0; k < 16 && m0 + k < M; ++k) dst[k] = (uint8_t)((w[r][k >> 2] >> ((k & 3) * 8)) & 0xFFu);
            }
        }
    }
}

// Raw SemanticKITTI voxel files -> labels.  The batch is one flat run of groups of 8 voxels (N % 8 == 0, so no group
// straddles two samples): a lane reads the group's 8 uint16 labels (16 bytes; the address may be only 2-byte aligned, so
// the load goes through memcpy and the compiler picks the instruction), one byte of each bit mask (MSB first: voxel 8g + j
// is bit 7 - j, io_data.unpack) and stores 8 label bytes, and 8 bytes of 0 / 1 when the occluded mask is given.  The LUT
// sits in LDS.  Raw values >= lut_len become 255 and are counted (the counter is zeroed by frustum_zero_kernel first).
constexpr int kMaxLut = 4096;

__global__ void __launch_bounds__(256) kitti_labels_kernel(const uint16_t* __restrict__ raw,
                                                           const uint8_t* __restrict__ invalid_bits,
                                                           const uint8_t* __restrict__ occluded_bits,
                                                           const uint8_t* __restrict__ lut, int lut_len,
                                                           uint2* __restrict__ target, uint2* __restrict__ occluded,
                                                           uint32_t* __restrict__ bad, long groups) {
    __shared__ uint8_t s_lut[kMaxLut];
    for (int i = threadIdx.x; i < lut_len; i += 256) s_lut[i] = lut[i];
    __syncthreads();
    uint32_t nbad = 0u;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long)gridDim.x * 256) {
        uint16_t v[8];
        __builtin_memcpy(v, raw + g * 8, 16);
        const uint32_t inv = invalid_bits[g];
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t r = v[j];
            const bool known = r < (uint32_t)lut_len;
            uint32_t lab = s_lut[known ? r : 0u];
            nbad += known ? 0u : 1u;
            if (!known || ((inv >> (7 - j)) & 1u)) lab = 255u;
            w[j >> 2] |= lab << ((j & 3) * 8);
        }
        target[g] = make_uint2(w[0], w[1]);
        if (occluded_bits) {
            const uint32_t occ = occluded_bits[g];
            uint32_t o[2] = {0u, 0u};
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j >> 2] |= ((occ >> (7 - j)) & 1u) << ((j & 3) * 8);
            occluded[g] = make_uint2(o[0], o[1]);
        }
    }
    if (nbad) atomicAdd(bad, nbad);
}

}  // namespace

extern "C" int occd_frustum_targets(const occd_frustum_args* a, void* stream) {
    if (!a || !a->cam_E || !a->cam_k || !a->target || !a->masks || !a->dists) return OCCD_EINVAL;
    if (a->batch <= 0 || a->batch > 65535 || (a->n_views != 1 && a->n_views != 2) || a->X <= 0 || a->Y <= 0 ||
        a->Z <= 0 || a->img_w <= 0 || a->img_h <= 0 || a->frustum_size < 1 || a->frustum_size > kMaxFrustum ||
        a->n_classes < 1 || a->n_classes > 255 || !(a->voxel_size > 0.0))
        return OCCD_EINVAL;
    const long N = (long)a->X * a->Y * a->Z;
    const int s = a->frustum_size, F = s * s;
    if (N > (1L << 31) - kVoxPerBlock || (long)F * a->n_classes > kMaxBins) return OCCD_EINVAL;
    FrustumP p;
    p.cam_E = a->cam_E;
    p.cam_k = a->cam_k;
    p.target = a->target;
    p.masks = a->masks;
    p.counts = reinterpret_cast<uint32_t*>(a->dists);
    for (int i = 0; i <= kMaxFrustum; ++i) {
        // helpers.py:205-216: ranges (i * 1.0 / size, (i * 1.0 + 1) / size), scaled by img_W / img_H
        p.sx[i] = i <= s ? ((double)i / (double)s) * (double)a->img_w : 0.0;
        p.sy[i] = i <= s ? ((double)i / (double)s) * (double)a->img_h : 0.0;
    }
    p.vox_size = a->voxel_size;
    for (int j = 0; j < 3; ++j) p.origin[j] = (float)a->vox_origin[j];
    p.X = a->X; p.Y = a->Y; p.Z = a->Z; p.N = (int)N;
    p.img_w = a->img_w; p.img_h = a->img_h;
    p.s = s; p.F = F; p.C = a->n_classes;
    p.vec = (N % kVoxPerThread) == 0;
    hipStream_t st = (hipStream_t)stream;
    const int ncnt = a->batch * F * a->n_classes;
    occd::ProfScope prof("frustum_targets", st, 0.0, (double)a->batch * N * (1.0 + F));
    hipLaunchKernelGGL(frustum_zero_kernel, dim3((unsigned)((ncnt + 255) / 256)), dim3(256), 0, st, p.counts, ncnt);
    const dim3 grid((unsigned)((N + kVoxPerBlock - 1) / kVoxPerBlock), (unsigned)a->batch);
    if (a->n_views == 2) hipLaunchKernelGGL(frustum_targets_kernel<2>, grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(frustum_targets_kernel<1>, grid, dim3(256), 0, st, p);
    hipLaunchKernelGGL(frustum_counts_to_float, dim3((unsigned)((ncnt + 255) / 256)), dim3(256), 0, st, p.counts, ncnt);
    return occd::check_launch();
}

extern "C" int occd_downsample_label(const uint8_t* in, uint8_t* out, int32_t batch, int32_t X, int32_t Y, int32_t Z,
                                     int32_t ds, void* stream) {
    if (!in || !out || batch <= 0 || X <= 0 || Y <= 0 || Z <= 0 || ds < 1 || ds > 64 || X % ds || Y % ds || Z % ds)
        return OCCD_EINVAL;
    const long n_out = (long)batch * (X / ds) * (Y / ds) * (Z / ds);
    // preprocess.py:118: empty_t = 0.95 * ds * ds * ds, evaluated left to right in float64
    const double empty_t = 0.95 * (double)ds * (double)ds * (double)ds;
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("downsample_label", st, 0.0, (double)batch * X * Y * Z + (double)n_out);
    hipLaunchKernelGGL(downsample_label_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, st, in, out, X, Y, Z, ds,
                       n_out, empty_t);
    return occd::check_launch();
}

extern "C" int occd_cp_mega_matrix(const uint8_t* coarse, uint8_t* out, int32_t batch, int32_t X, int32_t Y, int32_t Z,
                                   int32_t binary, void* stream) {
    if (!coarse || !out || batch <= 0 || batch > 65535 || X < 2 || Y < 2 || Z < 2) return OCCD_EINVAL;
    const long N = (long)X * Y * Z, M = (long)(X / 2) * (Y / 2) * (Z / 2);
    const long gy = (N + kRowsPerBlock - 1) / kRowsPerBlock;
    if (gy > 0x7FFFFFFFL || (M + kMegaTile - 1) / kMegaTile > 65535) return OCCD_EINVAL;
    const int R = binary ? 2 : 4;
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("cp_mega_matrix", st, 0.0, (double)batch * R * N * M);
    hipLaunchKernelGGL(cp_mega_kernel, dim3((unsigned)gy, (unsigned)((M + kMegaTile - 1) / kMegaTile), (unsigned)batch),
                       dim3(256), 0, st, coarse, out, X, Y, Z, N, M, binary ? 1 : 0);
    return occd::check_launch();
}

extern "C" int occd_kitti_labels(const uint16_t* raw, const uint8_t* invalid_bits, const uint8_t* occluded_bits,
                                 const uint8_t* lut, int32_t lut_len, uint8_t* target, uint8_t* occluded,
                                 int32_t* out_of_range, int32_t batch, int64_t N, void* stream) {
    if (!raw || !invalid_bits || !lut || !target || !out_of_range || batch <= 0 || N <= 0 || (N & 7) || lut_len < 1 ||
        lut_len > kMaxLut || (occluded_bits != nullptr) != (occluded != nullptr))
        return OCCD_EINVAL;
    // 2-byte labels and 8-byte stores: raw at an odd address or outputs off an 8-byte boundary are not supported
    if (((uintptr_t)raw & 1u) || ((uintptr_t)target & 7u) || ((uintptr_t)occluded & 7u) || ((uintptr_t)out_of_range & 3u))
        return OCCD_EINVAL;
    if (N > (1LL << 40) / batch) return OCCD_EINVAL;
    const long groups = (long)batch * (N / 8);
    long blocks = (groups + 255) / 256;
    if (blocks > 2048) blocks = 2048;                  // 8 workgroups per CU; the loop takes the rest
    hipStream_t st = (hipStream_t)stream;
    occd::ProfScope prof("kitti_labels", st, 0.0, (double)groups * (16.0 + 1.0 + 8.0 + (occluded ? 9.0 : 0.0)));
    hipLaunchKernelGGL(frustum_zero_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<uint32_t*>(out_of_range), 1);
    hipLaunchKernelGGL(kitti_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, st, raw, invalid_bits, occluded_bits, lut,
                       (int)lut_len, reinterpret_cast<uint2*>(target), reinterpret_cast<uint2*>(occluded),
                       reinterpret_cast<uint32_t*>(out_of_range), groups);
    return occd::check_launch();
}
