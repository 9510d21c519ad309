// Host walk of the chunked staging of dwconv2d_kernel (occdepth_amd/csrc/dwconv_stage.h), compiled and run by
// tests/test_dwconv_staged.py with the system C++ compiler.  The kernel's loads are unconditional and their results masked, so
// a read outside a plane changes no output: this program is the check for it.  For every geometry on the command line
//     planes H W k stride plane_stride
// and every (plane, workgroup, thread, pass) -- with 256 threads to a plane's block and, where a plane has at most 128 items,
// also with the 128 of a half workgroup -- it replays the kernel's staging loop through the header's own functions and asserts
//   * every issued 16-byte load lies inside [plane, plane + H * W),
//   * every tile element is written exactly once,
//   * with the bits the element-wise staging loop (the form before, re-stated here) puts there.
// Plane contents are distinct finite values; whatever lies between the planes of a padded pitch is NaN.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dwconv_stage.h"

static uint32_t bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

static long walk(int planes, int H, int W, int k, int stride, long xps) {
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int ph = std::max((Ho - 1) * stride + k - H, 0), pw = std::max((Wo - 1) * stride + k - W, 0);
    const int pad_t = ph / 2, pad_l = pw / 2;
    const int wq = (Wo + 3) / 4, nitems = Ho * wq, nblk = (nitems + 255) / 256;
    const int wp = occd::dw_tile_wp(Wo, k, stride), wp4 = wp / 4;
    const uint32_t magic = occd::dw_div_magic((uint32_t)wp4);
    std::vector<float> x((size_t)planes * xps, std::nanf(""));
    for (int p = 0; p < planes; ++p)
        for (int i = 0; i < H * W; ++i) x[(size_t)p * xps + i] = (float)(1 + p * H * W + i);     // (exact: < 2^24)
    long issued = 0;
    for (int p = 0; p < planes; ++p) {
        const float* xp = x.data() + (size_t)p * xps;
        for (int blk = 0; blk < nblk; ++blk) {
            // the rows of the tile as the kernel has always computed them
            const int item0 = blk * 256, oy_first = item0 / wq, oy_last = std::min(item0 + 255, nitems - 1) / wq;
            const int iy_first = oy_first * stride - pad_t, nrows = (oy_last - oy_first) * stride + k;
            const occd::DwRows tr = occd::dw_tile_rows(blk, Ho, Wo, k, stride, pad_t);
            if (tr.oy_first != oy_first || tr.iy_first != iy_first || tr.nrows != nrows) {
                std::printf("FAIL rows: plane %d block %d\n", p, blk);
                return -1;
            }
            const int nchunks = tr.nrows * wp4;
            // threads of the plane's block: 256, and the 128 of a half where two small planes share a workgroup
            for (int nt = 256; nt >= (nitems <= occd::kDwPairItems ? occd::kDwPairItems : 256); nt -= 128) {
            std::vector<uint32_t> tile((size_t)nrows * wp, 0xdeadbeefu);
            std::vector<int> count((size_t)nrows * wp, 0);
            for (int tid = 0; tid < nt; ++tid)
                for (int base = tid; base < nchunks; base += nt * occd::kDwPass) {
                    for (int i = 0; i < occd::kDwPass; ++i) {                 // the loads of a pass: all of them are issued
                        const int f = std::min(base + i * nt, nchunks - 1);
                        const occd::DwChunk ch = occd::dw_chunk(f, wp4, magic, tr.iy_first, pad_l, H, W);
                        ++issued;
                        if (ch.off < 0 || (long)ch.off + 4 > (long)H * W) {
                            std::printf("FAIL load outside the plane: plane %d block %d thread %d chunk %d: floats [%d, %d) of %d\n",
                                        p, blk, tid, f, ch.off, ch.off + 4, H * W);
                            return -1;
                        }
                    }
                    for (int i = 0; i < occd::kDwPass; ++i) {                 // the LDS writes of the pass
                        const int f = base + i * nt;
                        if (f >= nchunks) continue;
                        const occd::DwChunk ch = occd::dw_chunk(f, wp4, magic, tr.iy_first, pad_l, H, W);
                        uint32_t u[4] = {bits(xp[ch.off]), bits(xp[ch.off + 1]), bits(xp[ch.off + 2]), bits(xp[ch.off + 3])};
                        if (ch.sh != 0) {
                            uint32_t o[4];
                            occd::dw_shift(u, ch.sh, o);
                            std::memcpy(u, o, sizeof(u));
                        }
                        for (int t = 0; t < 4; ++t) {
                            tile[(size_t)4 * f + t] = ch.row_ok ? u[t] : 0u;
                            ++count[(size_t)4 * f + t];
                        }
                    }
                }
            for (int e = 0; e < nrows * wp; ++e) {
                const int r = e / wp, j = e - r * wp, iy = iy_first + r, ix = j - pad_l;
                const uint32_t ok = 0u - (uint32_t)(((unsigned)iy < (unsigned)H) & ((unsigned)ix < (unsigned)W));
                const float v = xp[(size_t)std::min(std::max(iy, 0), H - 1) * W + std::min(std::max(ix, 0), W - 1)];
                if (count[e] != 1 || tile[e] != (bits(v) & ok)) {
                    std::printf("FAIL tile: plane %d block %d element %d (row %d col %d): written %d times, %08x, expected %08x\n", p,
                                blk, e, r, j, count[e], tile[e], bits(v) & ok);
                    return -1;
                }
            }
            }
        }
    }
    return issued;
}

int main(int argc, char** argv) {
    if (argc < 7 || (argc - 1) % 6 != 0) {
        std::printf("usage: %s planes H W k stride plane_stride [...]\n", argv[0]);
        return 2;
    }
    for (int a = 1; a + 5 < argc; a += 6) {
        const int planes = std::atoi(argv[a]), H = std::atoi(argv[a + 1]), W = std::atoi(argv[a + 2]), k = std::atoi(argv[a + 3]);
        const int stride = std::atoi(argv[a + 4]);
        const long xps = std::atol(argv[a + 5]);
        if (planes < 1 || H < 1 || W < 4 || (k != 3 && k != 5) || (stride != 1 && stride != 2) || xps < (long)H * W) {
            std::printf("bad geometry %d %d %d %d %d %ld\n", planes, H, W, k, stride, xps);
            return 2;
        }
        const long n = walk(planes, H, W, k, stride, xps);
        if (n < 0) {
            std::printf("  in geometry planes %d H %d W %d k %d stride %d plane_stride %ld\n", planes, H, W, k, stride, xps);
            return 1;
        }
        std::printf("ok %dx%dx%d k%d s%d pitch %ld: %ld loads\n", planes, H, W, k, stride, xps, n);
    }
    return 0;
}
