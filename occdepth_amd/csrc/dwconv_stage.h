// Index arithmetic of the depthwise convolution's LDS tile (dwconv2d_kernel, csrc/nchw2d.hip) when it is staged in 16-byte
// chunks.  Plain C++ behind one macro, so that the same functions run in the kernel and in a host program: the kernel's loads
// are unconditional and their results are masked, so no GPU test can see a read outside a plane -- tests/test_dwconv_staged.py
// walks every (workgroup, thread, pass) of its geometries on the CPU through exactly these functions instead.
//
// The tile of a workgroup is [nrows][wp] floats, wp a multiple of 4; tile column j is image column j - pad_l, tile row r is image
// row iy_first + r; everything outside the image is zero.  Chunk f = r * (wp / 4) + m is tile columns 4m .. 4m+3 of row r and
// lies at float offset 4f of the tile.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define OCCD_DW_HD __host__ __device__ __forceinline__
#else
#define OCCD_DW_HD inline
#endif

namespace occd {

// Chunks in flight per thread while the tile is staged: thread `tid` of 256 owns chunks tid + 256 j; a pass issues the loads of
// kDwPass of them (a thread past the last chunk re-reads the last one) before it uses the first.
constexpr int kDwPass = 4;
// Planes of at most kDwPairItems items (one block each) may be run two to a workgroup: threads [0, 128) the first plane, [128, 256)
// the second, thread tid % 128 of a half owning chunks tid % 128 + 128 j of its plane's tile.
constexpr int kDwPairItems = 128;

// floats per tile row: the windows of the wq = ceil(Wo / 4) output quads of a row, the last one rounded up to whole float4s
OCCD_DW_HD int dw_tile_wp(int Wo, int k, int stride) {
    const int wq = (Wo + 3) / 4, span4 = ((3 * stride + k) + 3) / 4;
    return 4 * (wq - 1) * stride + 4 * span4;
}

// the input rows that the 256 items [256 block, 256 block + 255] of a plane read (an item: 4 adjacent outputs of one row)
struct DwRows {
    int oy_first, iy_first, nrows;
};
OCCD_DW_HD DwRows dw_tile_rows(int block, int Ho, int Wo, int k, int stride, int pad_t) {
    const int wq = (Wo + 3) / 4, nitems = Ho * wq, item0 = block * 256;
    const int last = item0 + 255 < nitems - 1 ? item0 + 255 : nitems - 1;
    DwRows t;
    t.oy_first = item0 / wq;
    t.iy_first = t.oy_first * stride - pad_t;
    t.nrows = (last / wq - t.oy_first) * stride + k;
    return t;
}

// n / d by one mul-hi for n * d < 2^32 (magic 0 encodes d == 1): the chunk index -> (row, chunk of the row) split
OCCD_DW_HD uint32_t dw_div_magic(uint32_t d) { return d <= 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + d - 1) / d); }
OCCD_DW_HD uint32_t dw_div(uint32_t n, uint32_t magic) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(n, magic) + (magic == 0u ? n : 0u);
#else
    return (uint32_t)(((uint64_t)n * magic) >> 32) + (magic == 0u ? n : 0u);
#endif
}

// Chunk f of a tile: ONE 16-byte load of the plane's floats [off, off + 4) -- always inside [0, H * W) for W >= 4: the row is
// clamped into [0, H), the start column into [0, W - 4].  Tile element t of the chunk is then loaded float sh + t where
// 0 <= sh + t < 4 and the row exists, else zero: sh = 0 in the interior, < 0 at the left edge, > 0 at (or beyond) the right one.
struct DwChunk {
    int off, sh;
    bool row_ok;
};
OCCD_DW_HD DwChunk dw_chunk(int f, int wp4, uint32_t wp4_magic, int iy_first, int pad_l, int H, int W) {
    const int r = (int)dw_div((uint32_t)f, wp4_magic), m = f - r * wp4;
    const int iy = iy_first + r, ix0 = 4 * m - pad_l;
    const int cy = iy < 0 ? 0 : iy > H - 1 ? H - 1 : iy;
    const int cx = ix0 < 0 ? 0 : ix0 > W - 4 ? W - 4 : ix0;
    DwChunk c;
    c.off = cy * W + cx;
    c.sh = ix0 - cx;
    c.row_ok = (unsigned)iy < (unsigned)H;
    return c;
}
// The four tile elements of a chunk from the bit patterns u[0..3] of its load: out[t] = u[sh + t], zero where sh + t is outside
// [0, 4).  Bit masks on sh == i - t (seven values), no select chain: hipcc turns `i == 0 ? u0 : i == 1 ? ...` into a branch tree.
OCCD_DW_HD void dw_shift(const uint32_t u[4], int sh, uint32_t out[4]) {
    uint32_t eq[7];                                        // eq[d + 3] = all ones when sh == d
    for (int d = -3; d <= 3; ++d) eq[d + 3] = 0u - (uint32_t)(sh == d);
    for (int t = 0; t < 4; ++t) {
        uint32_t v = 0u;
        for (int i = 0; i < 4; ++i) v |= u[i] & eq[i - t + 3];
        out[t] = v;
    }
}

}  // namespace occd
