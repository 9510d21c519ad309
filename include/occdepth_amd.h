/*
 * occdepth_amd.h -- C-ABI of libocc_hip.so, the MI355X (gfx950) kernel library
 * under the `occdepth.models` nn.Module surface.
 *
 * The reference (megvii-research/OccDepth) has NO FFI layer of its own: its hot
 * path is a graph of stock ATen ops called from Python.
 * Each entry point below therefore names the reference *Python* call site whose
 * ATen-op sequence it replaces; `occdepth_amd/hip.py` is the ctypes binding.
 *
 * Conventions
 *  - Python derives its binding (structures, prototypes, constants, ABI number) from this file at import
 *    (occdepth_amd/abi.py), so declarations stay within the subset it parses: block comments, `#define NAME integer`,
 *    `typedef struct T {...} T;` with plain `*` / `const` / `[N]` declarators, and function declarations.
 *  - plain pointers + ints only; all pointers are DEVICE pointers (fp32 unless
 *    noted) owned by the caller; nothing is retained after the call returns.
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream).  Every
 *    launch is asynchronous on that stream; no call synchronises the device.
 *  - return value: 0 (OCCD_OK) or a negative OCCD_E* code; occd_strerror()
 *    gives text.  The Python layer converts non-zero into RuntimeError.
 *  - voxel tensors are channels-last: row r = ((b*X + x)*Y + y)*Z + z holds the
 *    C channels of one voxel, `cs` floats apart (cs >= C, multiple of 4), at
 *    channel offset `coff` inside the row (so a tensor can be a channel slice
 *    of a wider concat buffer).  Channel pads must hold zeros.
 */
#ifndef OCCDEPTH_AMD_H
#define OCCDEPTH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCCD_OK 0
#define OCCD_EINVAL (-1)   /* bad argument / unsupported geometry          */
#define OCCD_ELAUNCH (-2)  /* hip launch / runtime error                   */
#define OCCD_ENOMEM (-3)   /* tile does not fit LDS                        */

#define OCCD_MAX_VIEWS 4
#define OCCD_MAX_SCALES 4

#define OCCD_ACT_NONE 0
#define OCCD_ACT_RELU 1
#define OCCD_ACT_SIGMOID 2
#define OCCD_ACT_RELU_PRE 3 /* act_out only: relu(conv + bias) + res1 + res2 */

/* ABI version, returned by occd_abi_version(); bumped whenever a struct below changes.  This is the one place the number
 * and its history are written: csrc/prof.cpp returns the macro and occdepth_amd/abi.py reads it.
 *  3: K10
 *  4: K11 pointwise GEMM, SE gate, depthwise pool / backward, softmax, lift backward + xcd_mode / feat_bstride
 *  5: K11s split-K hints, occd_upconv_gather_nchw (K12)
 *  6: K2b / K8b bf16-MFMA convolution forward + weight gradient, BN kernels
 *  7: occd_lift_proj_fwd (fused projection + frustum sample + lift), occd_pack_weights_bf16x3 + split mode of
 *     occd_conv3d_bf16_fwd
 *  8: occd_gemm_f32x3 (K16, row-major float32 GEMM with the 3-way bf16 split), K2s3 behind occd_conv3d_bf16_fwd dtype 2
 *  9: occd_gemm_args.res / scale_k (project convolutions on K16), occd_conv3d_fwd_phases
 * 10: strided (channels-last) ssc loss / confusion passes, occd_relation_bce_*, occd_depth_bce_*, occd_flosp_sample_bwd
 * 11: occd_gemm_args.act_a (sigmoid on A: CRP products on K16), peer-memory exchanges (occd_ipc_*, occd_bn_*_small_xchg),
 *     occd_stem_conv3x3_nchw, occd_depthnet_gate, occd_plane_reduce / occd_se_bwd
 * 12: x_plane_stride of occd_dwconv2d_pool_nchw
 * 13: occd_gemm_args.bias_n / stride_bias_n (column bias: CRP relation-logit convolutions on K16), occd_gemm_f32x3_splitk
 *     (K21), occd_se_gate_set_fused
 * 14: occd_graph_replace_memsets (captured memset nodes -> fill kernels)
 * 15: occd_pack_weights_f16x2 + dtype 3 of occd_conv3d_bf16_fwd (K2s3h, the two-term fp16 split of the head convolutions)
 * 16: occd_frustum_args, occd_frustum_targets, occd_downsample_label, occd_cp_mega_matrix (training targets on the GPU)
 * 17: occd_vox2pix_args, occd_vox2pix (batched device-side voxel -> pixel tables, flip included), occd_lift_proj_args.ida
 * 18: occd_optim_chunk, occd_clip_adamw_args, occd_grad_sumsq, occd_clip_adamw (gradient-norm clipping fused with AdamW)
 * 19: occd_kitti_labels (raw SemanticKITTI voxel files -> labels on the GPU)
 * 20: occd_optim_chunk.acc, occd_accum_adamw_args, occd_accum_clip_adamw (gradient accumulation over a window of
 *     micro-batches fused into clip + AdamW)
 * 21: occd_wino_packed_f16x2_bytes, occd_wino_pack_weights_f16x2, occd_wino_conv3x3_f16x2_fwd (K10h, the fused Winograd
 *     3x3 convolution on the two-term fp16 split)
 * 22: occd_confusion_region, occd_confusion_regions_args, occd_ssc_confusion_regions (SSC confusion counts by region --
 *     index box x camera FOV x byte masks, shared or per frame -- in one pass); added since without a change of any
 *     struct or prototype: occd_gemm_f16x2_packed_elems, occd_gemm_f16x2_pack and occd_gemm_args.pre = OCCD_GEMM_PRE_F16X2
 *     (the two-term fp16 split of the 2-D GEMMs that read pre-split weights: K16p, K21, K16 on the A image); likewise
 *     OCCD_FUSE_MAX_SOURCES, OccdFuseArgs, occd_fuse_store and occd_fuse_frames (temporal fusion of class probabilities
 *     over a sequence, csrc/fuse.hip): a new struct and new functions only; likewise OCCD_MAP_BRICK, OccdMapFrameArgs,
 *     OccdMapExtractArgs, occd_map_integrate, occd_map_brick_labels, occd_map_count and occd_map_extract (the sequence-level
 *     semantic voxel map, csrc/semantic_map.hip): two new structs and new functions only; likewise OccdMapRenderArgs and
 *     occd_map_render (K31, the sparse two-level ray cast over the map's bricks, csrc/map_render.hip): one new struct and
 *     one new function only; likewise OCCD_MAP_SAMPLE_EXCLUDE_SELF, OCCD_MAP_SAMPLE_KEEP_OWN, OccdMapSampleArgs and
 *     occd_map_sample (K32, the map read back into a frame's voxels, csrc/semantic_map.hip): one new struct and one new
 *     function only; likewise OccdMapMergeArgs and occd_map_merge (K33, the counter-wise saturating sum of two sets of
 *     bricks, csrc/semantic_map.hip): one new struct and one new function only; likewise OCCD_GEMM_KERNEL_* and
 *     occd_gemm_f32x3_route (the hint-0 kernel choice of occd_gemm_f32x3 as a host query): one new function only; likewise
 *     OccdVisibilityArgs and occd_frame_visibility (K34, the voxels of a frame the camera's pixel rays reach,
 *     csrc/visibility.hip) and OccdMapWeightedArgs, occd_map_integrate_weighted, OccdMapSampleWeightedArgs and
 *     occd_map_sample_weighted (votes of a weight per voxel, csrc/semantic_map.hip): three new structs and three new
 *     functions only; likewise OCCD_RAY_MAX_THRESHOLDS, OCCD_RAY_MAX_CLASSES, OCCD_RAY_UNKNOWN_*, OCCD_RAY_COUNTERS,
 *     OccdRayMetricArgs and occd_ray_metric (K35, the ray-wise counters of RayIoU, csrc/ray_metric.hip): one new struct
 *     and one new function only; likewise OCCD_RENDER_LOSS_ABS / _REL, OccdRenderLossArgs, occd_render_opacity,
 *     occd_render_depth_fwd, occd_render_depth_bwd_rays and occd_render_depth_bwd_voxels (K36, the depth-rendering loss,
 *     csrc/render_loss.hip): one new struct and four new functions only; likewise OCCD_EDT_MAX_CLASSES, OCCD_EDT_CHUNK,
 *     OccdEdtArgs, occd_edt_sq and occd_dist_metric (K37, the exact truncated squared distance transform of label volumes
 *     and the distance-tolerant score counters made of it, csrc/edt.hip): one new struct and two new functions only;
 *     likewise OCCD_SORT_TILE, OCCD_SORT_RADIX_BITS, OccdSortArgs and occd_sort_pairs_u32 (K38, the stable segmented
 *     radix sort, csrc/sort.hip) and OCCD_LOVASZ_*, OccdLovaszArgs, occd_lovasz_errors, occd_lovasz_ranks and
 *     occd_lovasz_bwd (the Lovasz-softmax loss on top of it, csrc/lovasz.hip): two new structs and four new functions only;
 *     likewise OCCD_MESH_*, OccdMeshArgs, occd_mesh_count, occd_mesh_emit, occd_mesh_heads and occd_mesh_weld (K39, the
 *     indexed quad mesh of a brick volume, csrc/mesh.hip): one new struct and four new functions only; likewise
 *     OCCD_CCL_*, OccdCclArgs, occd_ccl_segments, occd_ccl_roots, occd_ccl_compact and occd_ccl_filter (K40, connected
 *     components of a label volume, csrc/ccl.hip) and OccdCclPairArgs, occd_ccl_pair_marks, occd_ccl_pair_emit,
 *     occd_ccl_pair_heads and occd_ccl_pair_rows (the exact overlap counts of two segment volumes, sorted with
 *     occd_sort_pairs_u32): two new structs and eight new functions only; likewise
 *     occd_wino_conv3x3_f16x2_fwd_form (K10h with two cout blocks per work item, csrc/wino_conv2d.hip): one new function only */
#define OCCD_ABI_VERSION 22
int occd_abi_version(void);
const char* occd_strerror(int code);

/* ------------------------------------------------------------------------ *
 * K2: implicit-GEMM 3-D convolution on fp32 MFMA (v_mfma_f32_32x32x2_f32),
 * fused epilogue:  out = act_out( conv(act_in(in)) + bias + res1 + res2 ).
 *
 * Replaces, in eval mode with BatchNorm folded into (w, bias):
 *   nn.Conv3d + BatchNorm3d + ReLU + residual adds   occdepth/models/DDR.py:111-139
 *   ASPP / segmentation-head conv chains             occdepth/models/modules.py:40-46,158-175
 *   AvgPool3d + 1x1x1 conv side branches             occdepth/models/DDR.py:95-109 (as k=stride convs)
 *   nn.ConvTranspose3d(k3,s2,p1,op1)+BN+ReLU         occdepth/models/modules.py:278-296
 *     (run as 8 sub-pixel phases through the o_stride/o_off output scatter)
 *   1x1x1 relation logits, sigmoid + torch.bmm       occdepth/models/CRP3D.py:68-82
 *
 * `wpk` is the packed weight image produced by occd_pack_weights():
 *   wpk[tap][kt][nt][lane][q],  lane = kk*32 + j,  value =
 *   W[cout = nt*32 + j][cin = kt*8 + kk*4 + q][tap], tap = (kx*KY + ky)*KZ + kz,
 *   zero padded to Cin8 = ceil8(Cin) and 32*NT = ceil32(Cout).
 * ------------------------------------------------------------------------ */
typedef struct occd_conv3d_args {
    const float* in;    /* (B, X, Y, Z, in_cs)                               */
    const float* wpk;   /* packed weights, see above                         */
    const float* bias;  /* (32*NT) floats or NULL                            */
    const float* res1;  /* optional residual, laid out like `out`            */
    const float* res2;  /* optional second residual                          */
    float* out;         /* (B, OX, OY, OZ, out_cs)                           */
    int32_t batch;
    int32_t X, Y, Z;            /* input spatial dims                        */
    int32_t cin;                /* logical input channels (weights K extent) */
    int32_t in_cs, in_coff;
    int32_t cout;               /* logical output channels                   */
    int32_t out_cs, out_coff;
    int32_t res1_cs, res1_coff;
    int32_t res2_cs, res2_coff;
    int32_t kx, ky, kz;         /* kernel extent                             */
    int32_t sx, sy, sz;         /* stride                                    */
    int32_t dx, dy, dz;         /* dilation                                  */
    int32_t px, py, pz;         /* leading zero padding                      */
    int32_t Xo, Yo, Zo;         /* number of output positions computed       */
    int32_t OX, OY, OZ;         /* spatial dims of the out/res buffers       */
    int32_t o_stride_x, o_stride_y, o_stride_z; /* output voxel = o*stride+off */
    int32_t o_off_x, o_off_y, o_off_z;
    int32_t act_in;             /* OCCD_ACT_* applied to `in` on load        */
    int32_t act_out;            /* OCCD_ACT_NONE, OCCD_ACT_RELU (after the residual
                                   adds) or OCCD_ACT_RELU_PRE (before them)  */
    int32_t cout_store;         /* channels written per voxel (>= cout,
                                   multiple of 4, <= 32*NT); pads get 0+bias */
    int32_t tile_hint;          /* 0 = auto; else forces a kernel variant    */
} occd_conv3d_args;

int occd_conv3d_fwd(const occd_conv3d_args* a, void* stream);

/* The n in {1, 2, 4, 8} sub-pixel phases of ONE transposed convolution as one launch
 * (ConvTranspose3d(k3, s2, p1, op1) of the reference's Upsample blocks, occdepth/models/modules.py:278-296,
 * = 8 phase convolutions over tap subsets scattering to interleaved voxels).  a[0..n) may differ ONLY in
 * wpk, kx / ky / kz and o_off_*; OCCD_EINVAL otherwise.  Same arithmetic as n calls of occd_conv3d_fwd.   */
int occd_conv3d_fwd_phases(const occd_conv3d_args* a, int32_t n, void* stream);

/* Pack PyTorch-layout conv weights (Cout, Cin, KX, KY, KZ) [transposed=0] or
 * conv-transpose weights (Cin, Cout, KX, KY, KZ) [transposed=1] into `wpk`,
 * multiplying output channel c by scale[c] when scale != NULL (BN fold).
 * For a dynamic GEMM B operand (CRP bmm) pass w as (K=Cin, N=Cout) row-major
 * with layout=2.  Returns the number of floats written, or <0.              */
int64_t occd_packed_weight_floats(int32_t cout, int32_t cin, int32_t taps);
int occd_pack_weights(const float* w, const float* scale, float* wpk,
                      int32_t cout, int32_t cin, int32_t kx, int32_t ky, int32_t kz,
                      int32_t layout, void* stream);

/* ------------------------------------------------------------------------ *
 * K1a: FLoSP-Depth frustum sample.  For every voxel of the (A,B,C) grid and
 * every camera: voxel centre -> camera -> image (u, v, LID depth bin) -> ida ->
 * normalise by (W_img-1, H_img-1, D-1) -> trilinear grid_sample(align_corners=
 * False, zeros) of the (D, h, w) depth-probability frustum, plus the same sample
 * of an all-ones volume; mean over cameras where the ones-sample is > 0.
 * Replaces occdepth/models/flosp_depth/flosp_depth.py:561-602,
 * f2v/frustum_grid_generator.py:70-152, f2v/sampler.py:59-64.
 * ------------------------------------------------------------------------ */
typedef struct occd_flosp_args {
    const float* depth;     /* (B, n_cams, D, h, w) softmaxed depth bins      */
    const float* trans;     /* (B, n_cams, 4, 4)  lidar_to_cam @ grid_to_lidar */
    const float* proj;      /* (B, n_cams, 3, 4)  cam_to_img                   */
    const float* ida;       /* (B, n_cams, 4, 4)                               */
    const float* grids;     /* infer_mode: (n_cams, B, A, B, C, 3) precomputed
                               normalised grids, else NULL                    */
    float* out;             /* (B, A*B*C) */
    int32_t batch, n_cams;
    int32_t D, h, w;
    int32_t A, Bdim, C;     /* voxel grid dims (voxel_num)                    */
    float img_w, img_h;     /* final_dim (W, H) used by the normalisation     */
    float depth_min, depth_max;
    int32_t mean_mode;      /* 1 = "mean" aggregation, 0 = "sum"              */
} occd_flosp_args;

int occd_flosp_sample_fwd(const occd_flosp_args* a, void* stream);

/* Transpose of the frustum sample (what autograd computes through f2v/sampler.py:59-64's
 * F.grid_sample in training_step): gdepth (B, n_cams, D, h, w) = d loss / d depth given gout (B, A*B*C) = d loss / d out.
 * fwd.depth and fwd.out are not read (the sample is linear in the volume).  DETERMINISTIC: contributions are summed as
 * 64-bit fixed point with a power-of-two scale derived from max |gout| (both reductions are order-free), unlike
 * grid_sampler_3d_backward's float atomics.  workspace: >= 8 * (B n_cams D h w) + 8 bytes, 8-byte aligned, no
 * initialisation needed.                                                                                          */
typedef struct occd_flosp_bwd_args {
    occd_flosp_args fwd;
    const float* gout;
    float* gdepth;
    void* workspace;
    int64_t workspace_bytes;
} occd_flosp_bwd_args;
int occd_flosp_sample_bwd(const occd_flosp_bwd_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K1b: Stereo-SFA multi-scale lift.  Per voxel: for each 2-D scale gather the
 * projected pixel's C-vector from every view (mean over in-FOV pattern points),
 * fuse the views with the cosine-similarity weights, sum the scales, multiply by
 * depth_scale[voxel] * scale_const when depth_scale != NULL, write a
 * channels-last voxel row.
 * Replaces occdepth/models/SFA.py:12-106 called B x n_scales times from
 * occdepth/models/OccDepth.py:266-298, and the `x3ds * x3ds_depth * 100` of :339.
 * ------------------------------------------------------------------------ */
typedef struct occd_lift_args {
    /* feat[s][v]: (B, H_s*W_s, C) channels-last feature rows of view v, scale s */
    const float* feat[OCCD_MAX_SCALES][OCCD_MAX_VIEWS];
    int32_t feat_h[OCCD_MAX_SCALES], feat_w[OCCD_MAX_SCALES];
    int32_t feat_cs[OCCD_MAX_SCALES];     /* row stride (floats) of feat[s][*] */
    int32_t scale_div[OCCD_MAX_SCALES];   /* scale_2d: pixel // scale_div      */
    int32_t n_scales, n_views, batch;
    int32_t C;                            /* feature channels (multiple of 4)  */
    const int64_t* pix;                   /* (B, V, N, P, 2) int64 (x, y)      */
    const uint8_t* fov;                   /* (B, V, N, P) bool                 */
    int32_t N, P;
    const float* depth_scale;             /* (B, N) or NULL                    */
    float scale_const;                    /* 100.0 in the reference            */
    int32_t dimA, dimB, dimC;             /* n -> (a, b, c), n = (a*dimB+b)*dimC+c */
    int64_t row_a, row_b, row_c;          /* out row = a*row_a + b*row_b + c*row_c  */
    float* out;                           /* (B, rows, out_cs)                 */
    int64_t out_rows;                     /* rows per batch item               */
    int32_t out_cs;                       /* pads [C, out_cs) are zero-filled  */
    /* batch stride (floats) of feat[s][v]; 0 = dense (feat_h * feat_w * feat_cs).  Lets a view of a tensor that
     * interleaves the views (B, V, H, W, cs) be gathered in place.                                             */
    int64_t feat_bstride[OCCD_MAX_SCALES][OCCD_MAX_VIEWS];
    /* workgroup -> XCD placement of the single-pattern-point kernel (speed only, any value is correct):
     * 0 = dispatch order (columns of voxels dealt round-robin to the 8 XCDs), 1 = every XCD a contiguous range of the
     * flat voxel index, 2 = every XCD a contiguous (b, c) range inside every a-slab (needs dimB*dimC*LPV % 2048 == 0,
     * else falls back to 0).                                                                                    */
    int32_t xcd_mode;
} occd_lift_args;

int occd_lift_fwd(const occd_lift_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K14: one stride-1 DDR Bottleneck3D (occdepth/models/DDR.py:111-139 with BatchNorm folded) in two launches:
 *   o1 = relu(W1 x + b1); o2 = conv_z(o1) + b2; o3 = conv_y(relu(o2)) + b3 + o2; o4 = conv_x(relu(o3)) + b4 + o2 + o3;
 *   y = relu(W5 relu(o4) + b5 + x).       x, y: channels-last (B, X, Y, Z, cs) rows; C = channels of x and y, P = planes.
 * w: occd_bottleneck3d_weight_floats(C, P) floats = F(W1^T [C][P]) | b1 [P] | F(W2[0]) F(W2[1]) F(W2[2]) (per tap, [P in][P
 *    out]) | b2 | F(W3[.]) | b3 | F(W4[.]) | b4 | F(W5^T [P][C]) | b5 [C]   (tap k <-> offset (k - 1) * dilation), where
 *    F(W [KIN][MOUT]) is the matrix in MFMA fragment order: F[((t * MOUT/16 + m) * 64 + lane) * 4 + e] =
 *    W[16 t + 4 (lane >> 4) + e][16 m + (lane & 15)].   o2: workspace of B*X*Y*Z*P floats.
 * P in {16, 32}, C a multiple of 16, Z in {4, 8, 16} (a 16-voxel MFMA column block holds whole Z columns).
 * d0 / d1 / d2: dilation of the Z / Y / X convolution.
 * ------------------------------------------------------------------------ */
typedef struct occd_bneck_args {
    const float* x;
    float* y;
    float* o2;
    const float* w;
    int32_t batch, X, Y, Z, C, P;
    int32_t x_cs, x_coff, y_cs, y_coff;
    int32_t d0, d1, d2;
} occd_bneck_args;
int64_t occd_bottleneck3d_weight_floats(int32_t C, int32_t P);
int occd_bottleneck3d_fwd(const occd_bneck_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K15: pointwise (1x1x1) convolution / row GEMM on channels-last voxel rows:
 *   out[r][n] = act_out( sum_k act_in(a[r][k]) * w[k][n] + bias[n] (+ res[r][n]) ),   r < rows, k < K, n < N.
 * a / out / res: float32 rows with strides *_cs and channel offsets *_coff (a Vox or a channel slice of one); w: the
 * image occd_rows_gemm_pack makes of a dense [K][N] matrix (the (cin, cout) transpose of a 1x1x1 convolution weight with
 * the BatchNorm scale folded, or the mega-voxel rows of the CRP product, occdepth/models/CRP3D.py:80): MFMA fragment
 * records of occd_rows_gemm_packed_floats(K, N) floats.  K a multiple of 16, N a multiple of 4; w_stride is unused.
 * act_in: NONE / RELU / SIGMOID; act_out: NONE / RELU (after the residual) / RELU_PRE (before it).
 * ------------------------------------------------------------------------ */
typedef struct occd_rows_gemm_args {
    const float* a;
    const float* w;
    const float* bias;      /* N floats, padded to a multiple of 4, or NULL */
    const float* res;       /* or NULL */
    float* out;
    int64_t rows;
    int32_t K, N;
    int32_t a_cs, a_coff, out_cs, out_coff, res_cs, res_coff, w_stride;
    int32_t act_in, act_out;
} occd_rows_gemm_args;
int occd_rows_gemm_fwd(const occd_rows_gemm_args* a, void* stream);
int64_t occd_rows_gemm_packed_floats(int32_t K, int32_t N);
int occd_rows_gemm_pack(const float* w, float* wpk, int32_t K, int32_t N, int32_t w_stride, void* stream);

/* K16 (csrc/gemm_x3.hip): row-major float32 GEMM with the 3-way bf16 split of both operands (float32-level accuracy on the
 * bf16 matrix pipe):  C[b][m][n] = act(sum_k A[b][m][k] B[b][k][n] + bias[m]).  Replaces the library GEMMs behind the
 * reference's 2-D network call sites as this repo restates them (occdepth/models/unet2d.py:24-46 -- the first convolution of
 * a decoder level as nine low-resolution tap GEMMs --, :137-165 -- the Winograd-domain products of the second convolutions
 * at 1/8 and 1/16 --, and the geffnet MBConv expand 1x1 convolutions): torch.matmul / torch.bmm / F.conv2d there.
 * A: M x K with k contiguous (lda >= K, K % 8 == 0, 16-byte aligned rows); B: K x N with n contiguous (ldb >= N, N >= 4, any
 * dword alignment); C: M x N (ldc >= N).  stride_a == 0 shares A over the batch (weights).  bias: M floats or NULL.
 * act: OCCD_GEMM_ACT_NONE / _SWISH / _LEAKY (slope).  tile_hint: 0 = choose, 1 .. 5 = force a tile variant, 6 = the
 * wave-specialised 256 x 128 kernel, 7 = the 64 x 64 tile with the in-workgroup split-K, 8 = the panel-stationary kernel K16p
 * (pre = 1, K <= 848, no res / scale_k / act_a: a workgroup keeps 64 or 32 B columns over the whole K split in LDS and walks
 * the row tiles of the pre-split A image against them; hint 0 picks it for M >= 256) (tests / A-B).
 * Rows of C that start on 128-byte boundaries (ldc % 32 == 0, aligned base) are written 2.2x faster than rows 8 bytes off a
 * cache line (profiles/r05_store_alignment.txt): give intermediate results a padded ldc where the consumer takes a stride. */
#define OCCD_GEMM_ACT_NONE 0
#define OCCD_GEMM_ACT_SWISH 1
#define OCCD_GEMM_ACT_LEAKY 2
#define OCCD_GEMM_PRE_F16X2 4 /* occd_gemm_args.pre: A = the image of occd_gemm_f16x2_pack (two-term fp16 split, below) */
typedef struct occd_gemm_args {
    const float* A;
    const float* B;
    float* C;
    const float* bias;
    int32_t M, N, K, batch;
    int64_t lda, ldb, ldc;                 /* elements */
    int64_t stride_a, stride_b, stride_c;  /* elements between consecutive batch items */
    int32_t act;
    float slope;
    int32_t tile_hint;
    int32_t pre;                           /* 0: A, B float32; 1: A = occd_gemm_x3_pack(role 0) image; 2: B = role-1 image;
                                              3: float32 operands rounded to one bf16 term; OCCD_GEMM_PRE_F16X2: see below   */
    const float* res;                      /* optional (ABI 9): C += res[b][m][n] after bias / activation, laid out like C
                                              (ldc, stride_c): the skip connection of an MBConv project convolution      */
    const float* scale_k;                  /* optional (ABI 9): (batch, K) floats, B[b][k][:] is multiplied by scale_k[b][k]
                                              (rounded to float32, as the reference's x * gate) while it is staged: the
                                              squeeze-excite gate in front of the project convolution; pre must not be 2   */
    int32_t act_a;                         /* (ABI 11) 1: A[b][m][k] -> sigmoid(A[b][m][k]) while it is staged -- the relation
                                              products torch.bmm(sigmoid(P_logits), mega) of occdepth/models/CRP3D.py:80 as ONE
                                              batched launch over the relations; float32 A only (pre 0 / 2)                 */
    const float* bias_n;                   /* (ABI 13) optional: + bias_n[b][n] (one value per COLUMN) ahead of the activation --
                                              products whose ROWS are voxels and whose columns are output channels, e.g. the
                                              relation-logit 1x1x1 convolutions of occdepth/models/CRP3D.py:54-62 as one batched
                                              launch over the relations; occd_gemm_f32x3 only, not with tile_hint 6 / 8          */
    int64_t stride_bias_n;                 /* floats between the batch items of bias_n (0: shared)                              */
} occd_gemm_args;
int occd_gemm_f32x3(const occd_gemm_args* a, void* stream);
/* Which kernel occd_gemm_f32x3 launches for a problem, from shapes alone (host code, no device needed): the one rule the
 * launch itself follows, for callers that keep one weight image per route.  pre, tile_hint: as in occd_gemm_args; plain:
 * 1 = no res, no scale_k, no act_a, no bias_n.  *kernel = OCCD_GEMM_KERNEL_*; *variant = the panel width in 32-column
 * units (PANEL: 1 / 2) or the tile variant 0 .. 4 = 256 x 128, 128 x 128, 128 x 64, 64 x 64, 64 x 256 (TILE; WS is
 * always 0, KSPLIT always 3).  OCCD_EINVAL for shapes and hint / pre combinations occd_gemm_f32x3 rejects.              */
#define OCCD_GEMM_KERNEL_TILE 0   /* the barrier-phased tile kernels (K16)                   */
#define OCCD_GEMM_KERNEL_PANEL 1  /* K16p: the panel-stationary kernel on a pre-split A      */
#define OCCD_GEMM_KERNEL_WS 2     /* K16w: the wave-specialised 256 x 128 kernel             */
#define OCCD_GEMM_KERNEL_KSPLIT 3 /* the 64 x 64 tile with in-workgroup split-K              */
int occd_gemm_f32x3_route(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t pre, int32_t plain, int32_t tile_hint,
                          int32_t* kernel, int32_t* variant);
/* K21 (round 6), the skinny long-K GEMMs -- the MBConv project convolutions of the 1/16 and 1/32 EfficientNet stages,
 * `bn3(conv_pwl(x * se_gate)) + skip` (geffnet InvertedResidual behind occdepth/models/unet2d.py:188-196): K16p's
 * panel-stationary loop with K cut into `nz` chunks over the grid's z dimension, float32 partial tiles in `workspace`, and a
 * second launch that sums the chunks in index order (deterministic) and applies bias / activation / res.  Same operand
 * meaning as occd_gemm_f32x3 with pre = 1 (A = the role-0 image of occd_gemm_x3_pack; lda ignored), B float32 n-contiguous,
 * scale_k / res / bias / act optional; tile_hint and act_a must be 0.  occd_gemm_f32x3_splitk_plan proposes
 * (k16_per_z, nz, row_ranges) and the workspace size in floats (128-byte aligned buffer).  OCCD_EINVAL when a chunk would
 * not fit LDS (k16_per_z * 16 * 192 B <= 160 KB), the chunks do not tile K exactly, or the workspace is too small.        */
int occd_gemm_f32x3_splitk_plan(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t* k16_per_z, int32_t* nz,
                                int32_t* row_ranges, int64_t* workspace_floats);
int occd_gemm_f32x3_splitk(const occd_gemm_args* a, int32_t k16_per_z, int32_t nz, int32_t row_ranges, float* workspace,
                           int64_t workspace_floats, void* stream);
/* K16t, the "NT" form: C[b][m][n] = sum_k A[b][m][k] B[b][n][k], BOTH operands with k contiguous (lda, ldb >= K), any dword
 * alignment, any K: autograd's weight gradient of a pointwise convolution, dW = gy (Cout x HW) . x^T, on NCHW tensors as they
 * lie (training step, the geffnet MBConv 1x1 convolutions).  The reduction dimension is split over `act` (>= 1) workgroup
 * groups -- a weight gradient is a small matrix reduced over many pixels --: C receives batch x act partial matrices
 * (batch-major, stride_c elements apart) which the caller sums; occd_gemm_f32x3_nt_splits proposes `act` (every split must own
 * at least one 32-k step: pass exactly what it returns, or 1).  bias / pre must be NULL / 0; tile_hint 0 / 1 / 2.            */
int occd_gemm_f32x3_nt(const occd_gemm_args* a, void* stream);
int32_t occd_gemm_f32x3_nt_splits(int32_t M, int32_t N, int32_t K, int32_t batch);
/* A static operand (weights) split once into its three bf16 terms in MFMA fragment order, so the GEMM reads it straight
 * from L2 (no LDS, no split arithmetic): role 0 = an A operand (rows x K, k contiguous, ld >= K), role 1 = a B operand
 * (K x rows, "row" = column index contiguous, ld >= rows).  `out`: occd_gemm_x3_packed_elems(rows, K) bf16 per batch item,
 * consecutive; in_stride: float elements between the batch items of `w`.  With pre = 1 / 2 the packed operand's lda / ldb is
 * ignored and stride_a / stride_b counts bf16 elements (0 = shared over the batch).                                          */
int64_t occd_gemm_x3_packed_elems(int32_t rows, int32_t K);
int occd_gemm_x3_pack(const float* w, void* out, int32_t rows, int32_t K, int64_t ld, int32_t role, int32_t batch,
                      int64_t in_stride, void* stream);
/* The two-term fp16 split ("f16x2") of the GEMMs that read pre-split weights -- K16p, K21 and K16 on the A image -- with the
 * numerics of the head convolutions (OCCD_CONV_F16X2_HEAD): an A operand (rows x K, k contiguous, ld >= K) is packed once as
 * w'[m][k] = 2^k[m] w[m][k] (k[m]: the row's max |w'| in [2^13, 2^14); an all-zero row: k = 0), hi = fp16(w'),
 * lo = fp16(w' - hi), in the fragment order of the role-0 image above with two terms, [row tile 32][k16][hi, lo][lane][8],
 * followed by one float per row of the padded row tiles, fac[m] = 2^-(k[m] + 1).  occd_gemm_f16x2_packed_elems: 16-bit
 * elements per batch item, factors included (a multiple of 64); `out` 16-byte aligned.  occd_gemm_f16x2_pack returns
 * OCCD_EINVAL when a weight is not finite (it reads the factors back: a set-up call, not for a captured stream); the caller
 * keeps the three-term image.  A launch with pre = OCCD_GEMM_PRE_F16X2 (occd_gemm_f32x3 with tile_hint 0 .. 5 or 8, or
 * occd_gemm_f32x3_splitk; stride_a in 16-bit elements; no act_a, no bias_n) stages B as 2 x (after scale_k, in float32),
 * split hi + 2^-11 lo' in fp16, issues three v_mfma_f32_32x32x16_f16 per 16-k step -- (lo_a, hi_b), (2^-11 hi_a, lo'_b),
 * (hi_a, hi_b) -- and stores act(fac[m] * acc + bias[m]) (+ res).  Finite |B| >= 32760 overflow to non-finite outputs in
 * the columns they reach; routes and plans are those of pre = 1.                                */
int64_t occd_gemm_f16x2_packed_elems(int32_t rows, int32_t K);
int occd_gemm_f16x2_pack(const float* w, void* out, int32_t rows, int32_t K, int64_t ld, int32_t batch, int64_t in_stride,
                         void* stream);

/* The eval lift without its tables (SURVEY 8(f) N2 fused into K1b): the kernel projects every voxel
 * centroid itself (the arithmetic of occd_project_voxels: occdepth/data/utils/helpers.py:94-169, integer-exact), samples the
 * FLoSP depth frustum for the voxel (the arithmetic of occd_flosp_sample_fwd: flosp_depth.py:561-602) and applies
 * `* depth * scale_const` (OccDepth.py:339) -- no (B, V, N, 1, 2) int64 `projected_pix`, no `fov_mask`, no (B, N)
 * depth vector in HBM.  Single-point pattern (pattern_id 0), power-of-two scales and grid dims, <= 2 views.
 * lift.pix / lift.fov / lift.depth_scale are ignored; lift.dimA/B/C = the voxel grid (X, Y, Z) of the projection.
 * frustum.depth == NULL: no depth scaling (trans_2d_to_3d = "flosp"); frustum.out is ignored.                        */
typedef struct occd_lift_proj_args {
    occd_lift_args lift;
    const double* cam_E;    /* DEVICE (B, V, 4, 4) float64 extrinsics (lidar -> camera), the batch's T_velo_2_cam       */
    const double* cam_k;    /* DEVICE (B, V, 3, 3) float64 intrinsics, the batch's cam_k; fx, fy, cx, cy are rounded to
                               float32 inside the kernel, like the dataloader does (fusion.py:336-337)                */
    double voxel_size;      /* metres per voxel of the lifted grid (0.2 * project_scale)                              */
    float origin[3];        /* float32(vox_origin)                                                                    */
    int32_t img_w, img_h;
    occd_flosp_args frustum;
    const float* ida;       /* DEVICE (B, V, 4, 4) float32 image-space transforms (the batch's ida_mats) or NULL: a view
                               with ida[b][v][0][0] < 0 was flipped left-right, and every in-FOV pixel x is gathered at
                               img_w - 1 - x (kitti_dataset.py:384-390; the FOV itself is decided unflipped)         */
} occd_lift_proj_args;
int occd_lift_proj_fwd(const occd_lift_proj_args* a, void* stream);

/* Backward of occd_lift_fwd for single-point patterns (P = 1): what autograd computes through
 * SFA.forward x 4 scales and the `* depth * 100` of occdepth/models/OccDepth.py:266-298,339 in training_step.
 * gout (B, out_rows, out_cs) = d loss / d out, same rows as the forward output.  gfeat[s][v]: gradient maps with the
 * layout (and batch stride) of fwd.feat[s][v], ZEROED by the caller, accumulated with float atomics (summation order,
 * hence the last bits, vary from run to run).  gdepth (B, N) = d loss / d depth_scale, or NULL.                   */
typedef struct occd_lift_bwd_args {
    occd_lift_args fwd;
    const float* gout;
    float* gfeat[OCCD_MAX_SCALES][OCCD_MAX_VIEWS];
    float* gdepth;
} occd_lift_bwd_args;
int occd_lift_bwd(const occd_lift_bwd_args* a, void* stream);

/* voxel centroid -> pixel projection on the GPU instead of the dataloader's numba
 * `vox2pix` (occdepth/data/utils/helpers.py:94-169, fusion.py:203-217,336-337,518-522), pattern_id 0.
 * cam_E (4x4 row-major), cam_k (3x3), vox_origin (3) are small HOST arrays of doubles; outputs are device
 * tensors shaped like the batch entries `projected_pix_{s}` (N, 1, 2) int64 and `fov_mask_{s}` (N, 1) bool,
 * N = X*Y*Z voxels in (x, y, z) order; pix_z (N) float32 is optional.                              */
int occd_project_voxels(const double* cam_E_host, const double* cam_k_host, const double* vox_origin_host,
                        double voxel_size, int32_t X, int32_t Y, int32_t Z, int32_t img_w, int32_t img_h,
                        int64_t* pix, uint8_t* fov, float* pix_z, void* stream);

/* The same projection for a whole batch, calibration in DEVICE memory (capture-safe, no host sync): the tables the
 * reference's SemanticKITTI dataset ships, flip included.  For every (b, v) and voxel n = (x*Y + y)*Z + z:
 *   pix[b, v, n, 0, :], fov[b, v, n, 0], pix_z[b, v, n] = occd_project_voxels(cam_E[b, v], cam_k[b, v], ...)
 * then, when ida != NULL and ida[b, v, 0, 0] < 0 (img_transform(crop, flip=True), kitti_dataset.py:20-37), every x, in
 * the FOV or not, becomes img_w - 1 - x (kitti_dataset.py:388); the FOV is the unflipped one.  The rest of ida is
 * ignored.  Arbitrary grid dims.  Invalid arguments return OCCD_EINVAL without a launch. */
typedef struct occd_vox2pix_args {
    const double* cam_E;       /* (B, V, 4, 4) device float64, row major (lidar -> camera)                   */
    const double* cam_k;       /* (B, V, 3, 3) device float64 (fx, fy, cx, cy are rounded to float32)        */
    const float* ida;          /* (B, V, 4, 4) device float32, or NULL (no flip)                             */
    int64_t* pix;              /* (B, V, N, 1, 2) int64, 16-byte aligned                                     */
    uint8_t* fov;              /* (B, V, N, 1) bool                                                          */
    float* pix_z;              /* (B, V, N) float32 camera depth, or NULL                                    */
    double vox_origin[3];      /* rounded to float32 as vox2world does                                       */
    double voxel_size;
    int32_t batch, n_views, X, Y, Z;
    int32_t img_w, img_h;
} occd_vox2pix_args;
int occd_vox2pix(const occd_vox2pix_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * Layout / small fused helpers around the two big kernels.
 * ------------------------------------------------------------------------ */
/* (B, C, S) channel-first -> (B, S, cs) channels-last rows, zero pad [C, cs).
 * Feeds K1 from the torch 2-D decoder output (occdepth/models/unet2d.py:148-163)
 * and K2 from externally supplied (B,C,X,Y,Z) tensors.                        */
int occd_nchw_to_nhwc(const float* in, float* out, int32_t batch, int32_t C,
                      int64_t S, int32_t cs, void* stream);
/* inverse: (B, S, cs)[.., coff:coff+C] -> (B, C, S) */
int occd_nhwc_to_nchw(const float* in, float* out, int32_t batch, int32_t C,
                      int64_t S, int32_t cs, int32_t coff, void* stream);
/* softmax over n channels at [src_coff, src_coff+n) of each row, written to
 * [dst_coff, dst_coff+n) of the same-shaped dst rows, followed by dst_pad
 * zeros (cascade head: occdepth/models/modules.py:168-171 softmax + torch.cat). */
int occd_softmax_channels(const float* src, float* dst, int64_t rows,
                          int32_t src_cs, int32_t src_coff, int32_t dst_cs,
                          int32_t dst_coff, int32_t n, int32_t dst_pad, void* stream);

/* Cascade-head tail (occdepth/models/modules.py:166-173, after splitting conv_classes by linearity):
 *   out[v][o] = part[v][o] + sum_{tap<27, c<2} softmax(part[v+tap][occ_off : occ_off+2])[c] * wn[o][c][tap]
 * part: (B, X, Y, Z, part_cs) rows with the wide-half class logits at [0, nbr) and the 2 occupancy logits at
 * occ_off; wn: (nbr, 2, 3, 3, 3) = conv_classes.weight[:, planes:]; out: (B, X, Y, Z, out_cs); zero padding
 * applies to the softmax output.  VALU kernel (K = 54 is too thin for MFMA).
 * Only lanes [0, nbr) of an out row are written: lanes [nbr, out_cs) and whatever follows the last row are left
 * untouched.  The kernels are built for 3, 5 and 8 float4 groups of outputs (nbr <= 12, <= 20, <= 32) and load that
 * many floats of every part row, so part_cs must be at least 12, 20 or 32 (OCCD_EINVAL otherwise).  */
int occd_cascade_tail_fwd(const float* part, const float* wn, float* out, int32_t batch, int32_t X,
                          int32_t Y, int32_t Z, int32_t part_cs, int32_t occ_off, int32_t out_cs,
                          int32_t nbr, void* stream);

/* ------------------------------------------------------------------------ *
 * 2-D NCHW fused memory-bound helpers for the 2-D UNet (first step).
 * act: 0 none, 1 relu, 2 swish (x * sigmoid(x)), 3 leaky relu with `slope`.
 * ------------------------------------------------------------------------ */
/* y = act(x * scale[c] + shift[c]) + res   (res_first = 0)
 * y = act(x * scale[c] + shift[c] + res)   (res_first = 1)      x, res, y: (B, C, S); may alias.
 * BatchNorm2d(eval) + Swish / LeakyReLU / ReLU (+ residual) of the EfficientNet blocks
 * (third-party geffnet), unet2d.py:26-36 (conv+BN+LeakyReLU) and the DepthNet BasicBlocks
 * (flosp_depth.py:211-222).                                                  */
int occd_affine_act_nchw(const float* x, const float* res, float* y, const float* scale,
                         const float* shift, int32_t batch, int32_t C, int64_t S, int32_t act,
                         float slope, int32_t res_first, void* stream);

/* Backward of swish(x) = x * sigmoid(x) (the EfficientNet activation, geffnet behind occdepth/models/unet2d.py:175-190) in
 * one pass: gx = gy * s * (1 + x * (1 - s)), s = sigmoid(x); n contiguous floats, 16-byte aligned pointers.  The forward
 * is occd_affine_act_nchw with act = 2.                                                                             */
int occd_swish_bwd(const float* x, const float* gy, float* gx, int64_t n, void* stream);
/* y = softmax(x, dim=1) of a (B, C, S) map (S = H*W): the depth-bin softmax of FlospDepth.forward
 * (occdepth/models/flosp_depth/flosp_depth.py:548).                                         */
int occd_softmax_nchw(const float* x, float* y, int32_t batch, int32_t C, int64_t S, void* stream);
/* depthwise k x k (k = 3 or 5) convolution, x (B, C, H, W), w (C, 1, k, k), explicit top/left
 * zero padding (TensorFlow SAME), y (B, C, Ho, Wo) = act(conv * scale[c] + shift[c]).   */
int occd_dwconv2d_nchw(const float* x, const float* w, const float* scale, const float* shift,
                       float* y, int32_t batch, int32_t C, int32_t H, int32_t W, int32_t k,
                       int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                       int32_t act, void* stream);
/* Encoder stem (round 5; geffnet conv_stem + bn1 + act1 behind occdepth/models/unet2d.py:175-190): 3x3 convolution of the
 * 3-channel image x (B, 3, H, W) with w (cout, 3, 3, 3), stride 1 or 2, explicit top/left zero padding (TensorFlow SAME),
 * y (B, cout, Ho, Wo) = act(conv * scale[c] + shift[c]); act: 0 none, 1 relu, 2 swish.                              */
int occd_stem_conv3x3_nchw(const float* x, const float* w, const float* scale, const float* shift, float* y,
                           int32_t batch, int32_t H, int32_t W, int32_t cout, int32_t stride, int32_t pad_top,
                           int32_t pad_left, int32_t Ho, int32_t Wo, int32_t act, void* stream);
/* out (B, C + Cskip, H, W): [:, :C] = bilinear resize of x (B, C, h, w) with align_corners=True,
 * [:, C:] = skip (B, Cskip, H, W)  -- F.interpolate + torch.cat of unet2d.py:38-46.          */
int occd_upsample_bilinear_cat_nchw(const float* x, const float* skip, float* out, int32_t batch,
                                    int32_t C, int32_t Cskip, int32_t h, int32_t w, int32_t H,
                                    int32_t W, void* stream);
/* Channels-last twins for the bf16-mode training step (decoder levels as (B, H, W, C) pixel rows): the same resize + concat
 * with x (B, h, w, C), skip (B, H, W, Cskip), out (B, H, W, C + Cskip) dense rows, and the backward of the resized part as a
 * gather: gx (B, h, w, C) from gout (B, H, W, gout_cs) rows (its first C channels), the exact transpose of the forward.    */
int occd_upsample_bilinear_cat_nhwc(const float* x, const float* skip, float* out, int32_t batch, int32_t C, int32_t Cskip,
                                    int32_t h, int32_t w, int32_t H, int32_t W, void* stream);
/* Round 6: the same with output rows of out_cs >= C + Cskip floats, pad lanes written as zeros -- rows of ceil8(channels)
 * floats are consumed in place by the convolution kernels (the 163-channel concat of the full-resolution decoder level in
 * rows of 168: no strided copy into padded rows in front of the level's first convolution).                              */
int occd_upsample_bilinear_cat_nhwc_rows(const float* x, const float* skip, float* out, int32_t batch, int32_t C, int32_t Cskip,
                                         int32_t h, int32_t w, int32_t H, int32_t W, int32_t out_cs, void* stream);
int occd_upsample_bilinear_nhwc_bwd(const float* gout, float* gx, int32_t batch, int32_t C, int32_t gout_cs, int32_t h,
                                    int32_t w, int32_t H, int32_t W, void* stream);

/* conv3x3(pad 1)(bilinear_up(x))  ==  sum_t shift_t(bilinear_up(W_t . x)): given z (B, 9 * Cout, h, w) = the nine per-tap
 * channel mixings of the LOW-resolution map (one pointwise GEMM, tap t = ky * 3 + kx in channel block t), writes
 * out (B, Cout, H, W) = sum_t [inside] bilinear_{align_corners=True}(z_t)(oy + ky - 1, ox + kx - 1).  Replaces the
 * upsampled-channel part of the first convolution of a decoder level (occdepth/models/unet2d.py:24-46) -- the
 * (Cup + Cskip)-channel upsample+concat tensor is never formed.  z[b][ch][y][x] sits at b * z_batch_stride +
 * ch * z_channel_stride + y * w + x floats (0 = dense NCHW); (h*w*B, h*w) is the layout of ONE GEMM over all images.  */
int occd_upconv_gather_nchw(const float* z, float* out, int32_t batch, int32_t Cout, int32_t h, int32_t w,
                            int32_t H, int32_t W, int64_t z_channel_stride, int64_t z_batch_stride, void* stream);

/* The same with the level's remaining pieces fused, for <= 4 skip channels (the 1/1 level: the raw image):
 *   out = leaky_relu(gather(z) + conv3x3(skip, wskip, pad 1) + shift[co], slope)
 * skip (B, Cs, H, W), wskip (Cout, Cs, 3, 3) with the BatchNorm scale folded in, shift (Cout): the finished
 * `LeakyReLU(BN(conv(cat[up(x), skip])))` of `UpSampleBN` (unet2d.py:24-46) in one launch after the tap GEMM.     */
int occd_upconv_gather_skip_nchw(const float* z, const float* skip, const float* wskip, const float* shift, float* out,
                                 int32_t batch, int32_t Cout, int32_t Cs, int32_t h, int32_t w, int32_t H, int32_t W,
                                 int64_t z_channel_stride, int64_t z_batch_stride, float slope, void* stream);

/* Winograd F(2x2, 3x3) transforms for nn.Conv2d(k=3, s=1, p=1) of the 2-D decoder
 * (occdepth/models/unet2d.py:24-46).  T = B * ceil(H/2) * ceil(W/2) tiles, tile (b, ty, tx) -> row (b*th + ty)*tw + tx.
 *   input : x (B, Cin, H, W) -> V (16, T, Cin),  V[4i+j] = (B^T d B)[i][j] of the 4x4 patch at (2ty-1, 2tx-1), zero padded
 *   (caller): M[xi] (T, Cout) = V[xi] (T, Cin) . U[xi] (Cin, Cout),  U[4i+j][ci][co] = (G g[co][ci] G^T)[i][j]
 *   output: M (16, T, Cout) -> y (B, Cout, H, W) = act(scale[c] * (A^T M A) + shift[c]) (+ res before or after act;
 *           act codes of occd_affine_act_nchw).
 * A call covers the STRIP of tile rows [ty0, ty0 + ths) of every image (ths = ceil(H/2), ty0 = 0: the whole image):
 * T = B * ths * tw, row (b*ths + ty - ty0)*tw + tx.  Strips keep V / M of the high-resolution levels cache-sized.  */
int occd_wino_input_transform_nchw(const float* x, float* V, int32_t batch, int32_t Cin, int32_t H, int32_t W,
                                   int32_t ty0, int32_t ths, void* stream);
int occd_wino_output_transform_nchw(const float* M, const float* scale, const float* shift, const float* res,
                                    float* y, int32_t batch, int32_t Cout, int32_t H, int32_t W, int32_t ty0,
                                    int32_t ths, int32_t act, float slope, int32_t res_first, void* stream);

/* The same transforms in CHANNEL-MAJOR form, for the product with the weights as the LEFT operand:
 *   (caller): M^T[xi] (Cout, T) = U^T[xi] (Cout, Cin) . V^T[xi] (Cin, T) -- one occd_gemm_f32x3 launch of batch 16 with
 *             U^T as the image of occd_gemm_f16x2_pack (pre = OCCD_GEMM_PRE_F16X2), ldb = ldc = Tp.
 *   input : x (B, Cin, H, W) -> V^T (16, Cin, Tp);   output: M^T (16, Cout, Tp) -> y (B, Cout, H, W), epilogue as above.
 * Tp >= T is the row pitch in floats, a multiple of 32 (rows on 128-byte lines); columns [T, Tp) are neither written by the
 * input transform nor read by the output transform.  Whole images only (no strips).  Values, operation by operation, are
 * those of the _nchw pair.  OCCD_EINVAL: null x / V^T / M^T / y, Tp < T, Tp % 32 != 0, act outside 0 .. 3, or more than
 * 4 * 65535 channels.                                                                                             */
int occd_wino_input_transform_cm(const float* x, float* Vt, int32_t batch, int32_t Cin, int32_t H, int32_t W,
                                 int64_t Tp, void* stream);
int occd_wino_output_transform_cm(const float* Mt, const float* scale, const float* shift, const float* res,
                                  float* y, int32_t batch, int32_t Cout, int32_t H, int32_t W, int64_t Tp,
                                  int32_t act, float slope, int32_t res_first, void* stream);

/* K10: FUSED Winograd F(2x2, 3x3) convolution on the fp32 matrix pipe -- replaces
 * nn.Conv2d(k=3, s=1, p=1) + BatchNorm2d (eval) + activation of the 2-D decoder (occdepth/models/unet2d.py:24-46)
 * and the 3x3 convolutions of DepthNet / BasicBlock (occdepth/models/flosp_depth/flosp_depth.py:201-257):
 *   y = act( conv3x3(x, g * scale[co], pad 1) + shift[co] ) (+ res before or after act), x / y / res NCHW float32.
 * V = B^T d B is formed in registers from LDS-staged input patches, M stays in the MFMA accumulators, the output
 * transform runs in the epilogue: neither exists in memory (cf. the unfused transforms above).
 * upk: occd_wino_pack_weights(g (Cout, Cin, 3, 3), scale or NULL) -> occd_wino_packed_floats(Cout, Cin) floats,
 *      U = G g G^T * scale in MFMA A-fragment order [ceil(Cin/8)][16][ceil(Cout/32)][64 lanes][4].
 * shift: Cout floats or NULL.  act: codes of occd_affine_act_nchw (0 none, 1 relu, 2 swish, 3 leaky(slope)).
 * tile_hint: 0 = choose; 16 / 32 = tiles per wave along x (wave = 2 x 16 or 1 x 32 tiles).                     */
typedef struct occd_wino_args {
    const float* x;
    const float* upk;
    const float* shift;
    const float* res;
    float* y;
    int32_t batch, cin, cout, H, W;
    int32_t act, res_first, tile_hint;
    float slope;
} occd_wino_args;
int64_t occd_wino_packed_floats(int32_t cout, int32_t cin);
int occd_wino_pack_weights(const float* w, const float* scale, float* upk, int32_t cout, int32_t cin, void* stream);
int occd_wino_conv3x3_fwd(const occd_wino_args* a, void* stream);

/* K10h: the same convolution (same arguments, checks, epilogue and tile hints) on the f16 matrix pipe with the two-term
 * fp16 split of both operands -- three v_mfma_f32_32x32x16_f16 per Winograd position and 16 input channels, float32
 * accumulation; error against float64 within 2x of K10's (tests/test_wino_f16x2.py).  Finite activations with
 * |x| >= 8190 may give non-finite outputs (the transformed patch, |V| <= 4 max|x|, is staged as fp16(2 V)).
 * a->upk: the image of occd_wino_pack_weights_f16x2 (occd_wino_packed_f16x2_bytes(Cout, Cin) bytes, 16-byte aligned):
 *      fp16 [ceil(Cin/16)][16 positions][hi, lo][ceil(Cout/32)][64 lanes][8] of U' = 2^k[co] G g G^T scale (max |U'| of a
 *      cout in [2^13, 2^14)), A-fragment order, then ceil(Cout/32) * 32 floats 2^-(k[co] + 1).  The pack synchronises
 *      the stream and returns OCCD_EINVAL when a weight (times scale) is not finite (keep K10's image then).        */
int64_t occd_wino_packed_f16x2_bytes(int32_t cout, int32_t cin);
int occd_wino_pack_weights_f16x2(const float* w, const float* scale, void* upk, int32_t cout, int32_t cin, void* stream);
int occd_wino_conv3x3_f16x2_fwd(const occd_wino_args* a, void* stream);
/* K10h with the grid chosen by the caller.  max_workgroups:
 *    0  persistent workgroups, min(tile blocks x cout blocks, CUs of the device) of them, rounded down to a multiple of 8
 *       (one per XCD and round); workgroup g computes the items g, g + grid, ... -- a static assignment, no state on the
 *       device -- and requests the next item's first input patch while it stores the current one;
 *  k > 0  the same with min(items, k) workgroups; any k gives the same result;
 *   -1  one workgroup per item (the earlier kernel);
 * < -1  OCCD_EINVAL.
 *    0  with no more items than that grid has workgroups: the form -1 (nothing to hand over);
 * Every form gives the same bits.  occd_wino_conv3x3_f16x2_fwd(a, s) is the form -1, or the form 0 when OCCDEPTH_WINO_PERSIST=1
 * is in the environment of the first call (unset or "0": -1; any other value: OCCD_EINVAL from every call).  Both (and
 * occd_wino_conv3x3_fwd) need 20 H W < 2^32: the epilogue addresses the 5 output planes of a lane with 32-bit offsets.
 * The ABI number stays 22 although this export is new: no struct changed, and tests/test_metric_regions.py pins 22.  A
 * library without it fails at symbol lookup (hip.load() binds every export), not at the version check.                   */
int occd_wino_conv3x3_f16x2_fwd_ex(const occd_wino_args* a, int32_t max_workgroups, void* stream);
/* K10h with the work item chosen by the caller as well.  cout_blocks:
 *    1  an item is one block of 32 output channels and 128 tiles: occd_wino_conv3x3_f16x2_fwd_ex(a, max_workgroups, stream);
 *    2  the cout-pair form: an item is two neighbouring blocks of 32 output channels and 64 tiles, so the input patch of a
 *       tile block is fetched, transformed and split once for both (with an odd number of blocks the last pair computes
 *       one).  One workgroup per item only: max_workgroups must be -1, anything else is OCCD_EINVAL;
 * anything else: OCCD_EINVAL.  Same arguments, checks, weight image and profiler row; both forms give the same bits
 * (tests/test_wino_cout_pair.py).  Additive (OCCD_ABI_VERSION note).                                                     */
int occd_wino_conv3x3_f16x2_fwd_form(const occd_wino_args* a, int32_t max_workgroups, int32_t cout_blocks, void* stream);

/* Backward of the depthwise convolution (autograd of the geffnet conv_dw layers in training_step):
 *   data  : dx (B, C, H, W) from gy (B, C, Ho, Wo) and w (C, 1, k, k), same geometry arguments as the forward;
 *   weight: dw (C, 1, k, k) from x and gy; workspace: occd_dwconv2d_bwd_weight_workspace_floats(...) floats
 *           (per-workgroup partial sums, reduced in index order: deterministic).                                    */
int occd_dwconv2d_bwd_data_nchw(const float* gy, const float* w, float* dx, int32_t batch, int32_t C, int32_t H,
                                int32_t W, int32_t k, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho,
                                int32_t Wo, void* stream);
int64_t occd_dwconv2d_bwd_weight_workspace_floats(int32_t batch, int32_t C, int32_t k, int32_t Ho, int32_t Wo);
int occd_dwconv2d_bwd_weight_nchw(const float* x, const float* gy, float* dw, float* workspace, int32_t batch, int32_t C,
                                  int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad_top, int32_t pad_left,
                                  int32_t Ho, int32_t Wo, void* stream);
/* Depthwise convolution as above that ALSO leaves the squeeze-excite pooling behind: pool_part
 * (B*C, occd_dwconv2d_pool_blocks(Ho, Wo)) holds each workgroup's share of sum_{y,x} y[b][c] (fixed summation order).
 * occd_se_gate turns the partials into the gate  sigmoid(W_e swish(W_r mean + b_r) + b_e)  (B, C) of geffnet's
 * SqueezeExcite (conv_reduce (Cr, C), conv_expand (C, Cr)); r_scratch: B * Cr floats.  The gate is consumed by
 * occd_pw_conv_fwd's `gate` operand: x * gate never exists in memory.
 * x_plane_stride (ABI 12): floats between consecutive (b, c) input planes, 0 = H * W (dense); > H * W when x is the result of
 * an expand GEMM whose rows were put on a 128-byte pitch (rows of an odd pixel count are written 2.2x slower).            */
int32_t occd_dwconv2d_pool_blocks(int32_t Ho, int32_t Wo);
int occd_dwconv2d_pool_nchw(const float* x, const float* w, const float* scale, const float* shift, float* y,
                            float* pool_part, int32_t batch, int32_t C, int32_t H, int32_t W, int32_t k,
                            int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                            int32_t act, int64_t x_plane_stride, void* stream);
/* How occd_dwconv2d_nchw / occd_dwconv2d_pool_nchw stage the input rows of a workgroup in LDS: 1 (the default) in 16-byte
 * chunks with every load of the tile in flight at once, planes of at most 128 items two to a workgroup; 0 element by element
 * (the form before; also what W < 4 runs); 2 chunks with one plane per workgroup everywhere (measurement only).  y and
 * pool_part are bit-identical in all three.  OCCD_DW_STAGE=0 in the environment (read once) selects 0 as well; returns the
 * previous setting; a value outside 0..2 selects 1.  (Added without a change of any struct or prototype: no ABI bump.)  */
int32_t occd_dwconv2d_set_stage(int32_t form);
/* Squeeze-excite in TRAINING (autograd of geffnet's SqueezeExcite in training_step):
 *   forward : sums = occd_plane_reduce(x, NULL)  ->  occd_se_gate(sums, ..., nblk = 1, S)  ->  occd_affine_act_nchw (x * gate)
 *   backward: gg = occd_plane_reduce(gout, x)    ->  occd_se_bwd                           ->  occd_affine_act_nchw
 *             (gx = gout * gate + gm / S)
 * occd_plane_reduce: out[p] = sum_s a[p][s] (* b[p][s] when b != NULL) over `planes` dense planes of S floats, fixed order.
 * occd_se_bwd: from gg (B, C), the forward's gate (B, C), sums (B, C) and r = swish(Wr m + br) (B, Cr; occd_se_gate's
 * r_scratch), m = sums / S:  ds = gg g (1 - g);  gr = ds We;  z = Wr m + br;  dz = gr swish'(z)  and
 *   gm (B, C) = dz Wr,  gw_reduce (Cr, C) = dz^T m,  gb_reduce (Cr) = sum_b dz,  gw_expand (C, Cr) = ds^T r,  gb_expand (C) =
 *   sum_b ds;  dz_scratch: B * Cr floats.  batch <= 16.                                                                    */
int occd_plane_reduce(const float* a, const float* b, float* out, int64_t planes, int64_t S, void* stream);
int occd_se_bwd(const float* gg, const float* gate, const float* sums, const float* r, const float* w_reduce,
                const float* b_reduce, const float* w_expand, float* dz_scratch, float* gm, float* gw_reduce,
                float* gb_reduce, float* gw_expand, float* gb_expand, int32_t batch, int32_t C, int32_t Cr, int64_t S,
                void* stream);
/* DepthNet's camera-aware squeeze-excite gate in one launch (round 5; occdepth/models/flosp_depth/flosp_depth.py:201-257:
 * `Mlp(1, C, C)` of the scaled pixel size -> `SELayer(C)`):
 *   gate[i][c] = sigmoid(We relu(Wr (W2 relu(w1 s_i + b1) + b2) + br) + be),   i = 0 .. images-1
 * s_i = sps[i] (infer_mode) or factor * |(1 / K_i[0][0], 1 / K_i[1][1])| from `intrins` (row-major matrices with >= 6
 * floats per image, `intr_stride` floats apart: element [1][1] at offset 5 -- the (B, n_cams, 4, 4) intrinsics of the
 * batch); exactly one of sps / intrins is non-NULL.  w1 (C), w2 / wr / we (C, C) row major, biases (C).          */
int occd_depthnet_gate(const float* sps, const float* intrins, int64_t intr_stride, float factor, const float* w1,
                       const float* b1, const float* w2, const float* b2, const float* wr, const float* br,
                       const float* we, const float* be, float* gate, int32_t images, int32_t C, void* stream);
int occd_se_gate(const float* pool_part, const float* w_reduce, const float* b_reduce, const float* w_expand,
                 const float* b_expand, float* r_scratch, float* gate, int32_t batch, int32_t C, int32_t Cr,
                 int32_t nblk, int64_t S, void* stream);
/* Round 6: an opt-in ONE-launch form of occd_se_gate (reduce + expand with an in-kernel hand-off through self-validating
 * agent-scope words: csrc/se2d.hip se_fused_kernel) for C <= 4096, Cr % 4 == 0, Cr <= 192, batch * Cr <= 4096 -- bit-identical
 * to the two launches (r_scratch receives the squeezed activations in both forms: occd_se_bwd reads them).  Measured equal in
 * the frame and slower per launch (14.5 against 11.8 us), so the default stays two launches; this switch (or OCCD_SE_FUSED=1
 * in the environment) selects the one-launch kernel; returns the previous setting.                                       */
int32_t occd_se_gate_set_fused(int32_t on);

/* Round 6 (ABI 14): captured-graph hygiene.  `graph` is a hipGraph_t that stream capture produced and that has NOT been
 * instantiated yet (torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph()).  Every MEMSET node is replaced by a KERNEL node
 * with the same destination, value, extent and edges: on ROCm 7.2 / gfx950 a captured hipMemsetAsync fills with its value on
 * the first launch of the instantiated graph only and with a stale pattern afterwards (tools/probe_graph_memset.py), which
 * leaves ATen's multi-block reductions -- they zero their semaphores that way -- without output on replays.  No reference
 * counterpart (scripts/train.py:176-206 launches the step eagerly).  Returns the number of nodes replaced (>= 0) or a
 * negative OCCD_E* code; element sizes 1 / 2 / 4, flat and pitched extents.                                              */
int occd_graph_replace_memsets(void* graph);

/* K11: pointwise (1x1) convolution on NCHW maps as a GEMM on the fp32 matrix pipe with the
 * EfficientNet / decoder epilogue fused -- replaces conv1x1 + BatchNorm2d (eval) + Swish (+ squeeze-excite gate on the
 * input, + MBConv skip add) of the geffnet blocks behind occdepth/models/unet2d.py:175-190, the `resize_output_1_s`
 * convolutions of DecoderBN (unet2d.py:137-165) and DepthNet.depth_pred (flosp_depth/flosp_depth.py:225-227):
 *   y[b][co][n] = act( sum_ci (w[co][ci] * scale[co]) * (x[b][ci][n] * gate[b][ci]) + shift[co] ) (+ res[b][co][n])
 * x (B, Cin, N), y / res (B, Cout, N), N = H*W; gate (B, Cin) or NULL; shift (Cout) or NULL; act codes as above.
 * wpk: occd_pw_pack_weights(w (Cout, Cin), scale or NULL) -> occd_pw_packed_floats(Cout, Cin) floats in MFMA
 *      A-fragment order [ceil(Cin/8)][ceil(Cout/32)][64 lanes][4].  tile_hint: 0 = choose, 1..6 = fixed streaming
 *      variant, 7..12 = fixed split-K variant (K11s: the waves of a workgroup split Cin, for maps of few pixels).
 * out_nhwc_cs != 0: y is written pixel-major, y[b][n][co] in rows of out_nhwc_cs >= Cout floats (pad written as zeros)
 *      -- the layout occd_lift_fwd gathers from, so the decoder's 1x1 heads feed the lift without a transpose pass
 *      (no gate / res in this mode).                                                                              */
typedef struct occd_pw_args {
    const float* x;
    const float* wpk;
    const float* shift;
    const float* gate;
    const float* res;
    float* y;
    int64_t N;
    int32_t batch, cin, cout;
    int32_t act, tile_hint;
    float slope;
    int32_t out_nhwc_cs;
} occd_pw_args;
int64_t occd_pw_packed_floats(int32_t cout, int32_t cin);
int occd_pw_pack_weights(const float* w, const float* scale, float* wpk, int32_t cout, int32_t cin, void* stream);
int occd_pw_conv_fwd(const occd_pw_args* a, void* stream);

/* SURVEY 8(f) row N4 (first step): out[row] = lut[argmax_c x[row][coff + c]] (first maximum wins; lut may
 * be NULL) as uint16 -- replaces the host softmax + numpy argmax of scripts/generate_output.py:94-95 and the
 * learning_map_inv lookup of scripts/generate_kitti_submission.py:74-85.                               */
int occd_argmax_channels(const float* x, int64_t rows, int32_t cs, int32_t coff, int32_t C,
                         const uint16_t* lut, uint16_t* out, void* stream);

/* ------------------------------------------------------------------------ *
 * Headless voxel renderer (csrc/render.hip; csrc/raycast.h holds the same traversal for the other ray-cast kernels):
 * ray-cast label volumes to images, one launch for batch x n_views x H x W pixels, one thread per pixel -- the GPU
 * counterpart of the reference's mayavi / open3d viewers
 * (scripts/visualization/kitti_vis_pred.py, NYU_vis_pred.py), which need a display.  Added without an ABI bump: entries
 * and structures only, every older caller stays valid.  No atomics, no allocation, no host sync (capture-safe).
 *
 * Ray of pixel (u, v) of a view, in GRID units (one voxel = 1; the volume is the box [0,X] x [0,Y] x [0,Z]):
 *   origin = o0 + (u + 1/2) ou + (v + 1/2) ov,   dir = d0 + (u + 1/2) du + (v + 1/2) dv          (float32, no fma)
 * -- a pinhole camera (constant origin; scale dir so that t is camera depth), an orthographic view (constant dir) or a
 * mirrored one (negated du) alike; the kernel knows nothing about calibration.
 * Traversal: slab test against the box (a zero direction component is `parallel`: inside or outside by the origin; a
 * non-finite ray misses); t_enter = max(largest near-slab t, 0); entry face = the axis of that slab (lowest axis on
 * ties), 3 when t_enter = 0; first voxel = clamp(floor(origin + dir t_enter), 0, dims - 1); then Amanatides-Woo steps
 * with tmax_a = ((index_a + (dir_a > 0)) - origin_a) * (1 / dir_a) recomputed from the boundary at every step, the lowest
 * axis winning ties; the stepped axis becomes the face and t that tmax; the walk ends at the first visible voxel, when
 * the index leaves the grid, when no boundary is left to cross, or after X + Y + Z + 3 steps (never reached: every step
 * moves one index one way).  Every index is in range before its load.
 * Visible: class mode (target == NULL) 0 < label < 255.  Error mode: target == 255 is transparent; else visible when the
 * prediction (0 < label < 255) or the target (!= 0) is occupied.
 * Colour (integers): c = palette[row] * shade[face] >> 8, shade = {160, 208, 256, 256}; c = c / 3 * 2 when fov != NULL and
 * fov[voxel] == 0; row = min(label, n_palette - 1) in class mode; in error mode the last three palette rows are {occupied
 * with the wrong class, false positive, false negative} and a correct voxel takes row min(label, n_palette - 4).  With a
 * background image: hit -> (alpha c + (256 - alpha) bg) >> 8, miss -> bg; without: miss -> bg_colour.  Pixels of the
 * (H, W) canvas outside a view's own view_w x view_h rectangle (0 = the whole canvas) are misses.
 * OCCD_EINVAL without a launch: NULL labels / views / palette / rgb, non-positive sizes, X Y Z > 2^31 - 1, label_bytes or
 * (with a target) target_bytes other than 1 or 2, n_views > OCCD_RENDER_MAX_VIEWS, alpha outside 0..256, n_palette < 1 (4
 * in error mode), a view rectangle larger than the canvas.
 * ------------------------------------------------------------------------ */
#define OCCD_RENDER_MAX_VIEWS 8
typedef struct OccdRenderView {
    float o0[3], ou[3], ov[3];
    float d0[3], du[3], dv[3];
} OccdRenderView;

typedef struct OccdRenderArgs {
    const void* labels;            /* (B, X, Y, Z) uint8 / uint16 prediction                                  */
    const void* target;            /* (B, X, Y, Z) uint8 / uint16, or NULL: class mode                        */
    const uint8_t* fov;            /* (B, X, Y, Z) bytes, 0 = outside the camera's FOV (dimmed), or NULL      */
    const OccdRenderView* views;   /* (B, n_views) device                                                     */
    const uint8_t* palette;        /* (n_palette, 3) device                                                   */
    const uint8_t* background;     /* (B, n_views, H, W, 3), or NULL                                          */
    uint8_t* rgb;                  /* (B, n_views, H, W, 3)                                                   */
    int32_t* hit;                  /* (B, n_views, H, W) voxel index (x Y + y) Z + z or -1, or NULL           */
    uint8_t* face;                 /* (B, n_views, H, W) 0 / 1 / 2 = x / y / z, 3 = started inside or miss, or NULL */
    float* depth;                  /* (B, n_views, H, W) t at the hit, +inf on a miss, or NULL                */
    int32_t batch, n_views, H, W;
    int32_t X, Y, Z;
    int32_t label_bytes, target_bytes;
    int32_t n_palette, alpha;
    int32_t view_w[OCCD_RENDER_MAX_VIEWS], view_h[OCCD_RENDER_MAX_VIEWS];
    uint8_t bg_colour[4];
} OccdRenderArgs;
int occd_render_voxels(const OccdRenderArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * Stereo depth targets from a rectified image pair (csrc/stereo.hip): census transform, semi-global matching over the
 * four axis-aligned paths, winner-take-all with three validity checks, sub-pixel fit, depth = f B / disparity -- the
 * `gt_depth` map of use_stereo_depth_gt, which the reference reads from 16-bit PNGs an external stereo network wrote
 * (kitti_dataset.py:40-44, :338-348).  Added without an ABI bump: entries and one structure only, every older caller
 * stays valid.  No atomics, no allocation, no host sync, no dependency between workgroups of a launch (capture-safe);
 * every index is in range before its load.  Diagonal paths, median / speckle filtering and an adaptive P2 are not built.
 *
 * Per frame b: gray images L = gray[b][0], R = gray[b][1] (H, W) uint8, D = max_disp disparities, and a direction s:
 * s = -1 when ida != NULL and ida[b][0][0][0] < 0 (a frame the loader mirrored: left pixel x matches right pixel x + d),
 * else s = +1 (it matches x - d).  One launch may hold frames of both kinds.
 * Gray (occd_stereo_census with img != NULL; float32, no fma): u_c = clamp(rint((img_c std[c] + mean[c]) 255), 0, 255),
 *   g = (77 u_R + 150 u_G + 29 u_B + 128) >> 8, written to `gray`.  With img == NULL `gray` is the input.
 * Census: window 9 wide x 7 tall, coordinates clamped to the image; the 62 neighbours row-major from the top-left,
 *   skipping the centre; bit k of the 64-bit word is set when neighbour k < centre.
 * Cost: C(y, x, d) = popcount(cl[y, x] ^ cr[y, x - s d]) when 0 <= x - s d < W, else 62 (never stored).
 * Paths, four (left to right, right to left, downwards, upwards): the first pixel of a path has L = C; after it
 *   L(p, d) = C(p, d) + min(L(q, d), L(q, d - 1) + P1, L(q, d + 1) + P1, m(q) + P2) - m(q),  m(q) = min_k L(q, k),
 *   q the previous pixel of the path, the d - 1 / d + 1 terms absent at the ends of the range.  L <= 62 + P2 <= 255.
 *   S = the sum of the four paths (uint16, <= 4 (62 + P2)).
 * Winner: d0 = argmin_d S (lowest d on ties), best = S[d0].
 * Flags (bit 0, 1, 2), all three required: unique 100 best <= U S2 with S2 = min S[d] over |d - d0| > 1;
 *   consistent xr = x - s d0 inside the image and |dR(y, xr) - d0| <= 1, where dR(y, x') = argmin_d S(y, x' + s d, d)
 *   over the d that stay inside the image (lowest d on ties); inner 1 <= d0 <= D - 2.
 * Sub-pixel (float32): a = S[d0 - 1], b = S[d0 + 1], den = 2 (a + b - 2 best), sub = den > 0 ? (float)(a - b) /
 *   (float)den : 0; disp = (float)d0 + sub where flags == 7, else 0.
 * Depth (occd_stereo_depth): fB = (float)(cam_k[b][0][0][0] * sqrt((tx tx + ty ty) + tz tz)) in float64 on the device,
 *   t = cam_E[b][0][:3, 3] - cam_E[b][1][:3, 3] (view 0 is taken to be the left camera of the rectified pair);
 *   depth = disp > 0 ? fB / disp : 0.
 * Workspace: occd_stereo_workspace_bytes(batch, H, W, max_disp) bytes, 256-byte aligned, owned by the caller (four byte
 *   volumes (B, 4, H, W, D), one per path direction, and the dR map); its content is scratch.
 * OCCD_EINVAL without a launch: a NULL structure or a NULL pointer the entry needs (census: gray, census; sgm: census,
 *   workspace, S, d0, flags, disp; depth: disp, depth, cam_k, cam_E), non-positive batch / H / W (or batch > 32767,
 *   H > 65535, H W > 2^29), max_disp no multiple of 64 or outside 64..256, P1 < 0, P1 > P2, P2 > 193, uniqueness outside
 *   1..100, ida with ida_views < 1, calib_views < 2 (depth).  occd_stereo_workspace_bytes returns OCCD_EINVAL likewise.
 * ------------------------------------------------------------------------ */
typedef struct OccdStereoArgs {
    const float* img;              /* (B, 2, 3, H, W) normalised float32, or NULL: `gray` is the input          */
    uint8_t* gray;                 /* (B, 2, H, W)                                                              */
    void* census;                  /* (B, 2, H, W) 64-bit words                                                 */
    const float* ida;              /* (B, ida_views, 4, 4) float32, or NULL: no frame is mirrored               */
    void* workspace;               /* occd_stereo_workspace_bytes(...) bytes                                    */
    uint16_t* S;                   /* (B, H, W, D) summed path costs                                            */
    int32_t* d0;                   /* (B, H, W) winner                                                          */
    uint8_t* flags;                /* (B, H, W) 1 unique | 2 consistent | 4 inner                               */
    float* disp;                   /* (B, H, W) sub-pixel disparity, 0 = invalid                                */
    const double* cam_k;           /* (B, calib_views, 3, 3) float64                                            */
    const double* cam_E;           /* (B, calib_views, 4, 4) float64, world -> camera                           */
    float* depth;                  /* (B, H, W) metres, 0 = invalid                                             */
    int32_t batch, H, W, max_disp;
    int32_t p1, p2, uniqueness;
    int32_t ida_views, calib_views;
    float mean[3], std[3];
} OccdStereoArgs;
int64_t occd_stereo_workspace_bytes(int32_t batch, int32_t H, int32_t W, int32_t max_disp);
int occd_stereo_census(const OccdStereoArgs* a, void* stream);
int occd_stereo_sgm(const OccdStereoArgs* a, void* stream);
int occd_stereo_depth(const OccdStereoArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K8: weight gradient of a 3-D convolution (training step):
 *   dw[co][ci][kx][ky][kz] = sum_{b,xo,yo,zo} gy[b,xo,yo,zo][co] * x[b, xo*sx - px + kx*dx, ...][ci]
 * -- what autograd computes for nn.Conv3d.weight in the reference's training step
 * (occdepth/models/OccDepth.py:535-537 -> every nn.Conv3d of models/DDR.py, modules.py, CRP3D.py).  The data
 * gradient needs no kernel of its own: it is occd_conv3d_fwd on gy with the flipped, channel-transposed weights
 * (stride 1) or the sub-pixel phases of the transposed convolution (stride > 1).
 * x, gy: channels-last fp32 like occd_conv3d_args; dw: PyTorch weight layout, overwritten.
 * `workspace` must hold occd_conv3d_wgrad_workspace_floats() floats (partial tiles; summed in a fixed order,
 * so the result is deterministic).  At most 28 taps.                                                           */
typedef struct occd_conv3d_wgrad_args {
    const float* x;      /* (B, X, Y, Z, x_cs) input of the convolution        */
    const float* gy;     /* (B, Xo, Yo, Zo, gy_cs) gradient w.r.t. its output  */
    float* dw;           /* (cout, cin, kx, ky, kz)                            */
    float* workspace;
    int64_t workspace_floats;
    int32_t batch;
    int32_t X, Y, Z, cin, x_cs, x_coff;
    int32_t Xo, Yo, Zo, cout, gy_cs, gy_coff;
    int32_t kx, ky, kz, sx, sy, sz, dx, dy, dz, px, py, pz;
} occd_conv3d_wgrad_args;
int64_t occd_conv3d_wgrad_workspace_floats(const occd_conv3d_wgrad_args* a);
int occd_conv3d_wgrad(const occd_conv3d_wgrad_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K13: training-mode BatchNorm (+ activation + residual) as HBM-bound passes, forward and backward
 * (torch.nn.BatchNorm{2,3}d / SyncBatchNorm in training mode: occdepth/models/DDR.py:111-139, modules.py:40-46,158-175,
 * 278-296, unet2d.py:24-46; scripts/train.py:179 `sync_batchnorm=True`).
 *   layout 0: channels-last rows (`rows` rows of `*_cs` elements, channels at `*_coff`; dtype 0 fp32 / 1 bf16)
 *   layout 1: NCHW planes (`batch` x C planes of S fp32 elements; the *_cs / *_coff fields are ignored)
 * forward : occd_bn_stats (x -> partial) ; occd_bn_stats_combine (partial -> packed[2C+1] float64 =
 *           [n mean_c, M2_c + n mean_c^2, n], the form that sums over ranks) ; [all-reduce packed] ; occd_bn_finish
 *           (packed -> mean, invstd, a = gamma invstd, b = beta - mean a, running statistics with the unbiased variance,
 *           num_batches_tracked += 1) ; occd_bn_apply: out = act(x a + b [+ res if res_first]) [+ res if !res_first],
 *           act = 0 none / 1 relu / 2 swish / 3 leaky-relu(slope); `cw` (>= ceil4(C), rows layout) channels are written
 *           per row, those >= C as zeros.
 * backward: occd_bn_bwd_reduce (g = gy act'(pre), pre from `y`'s sign when y != NULL else x a + b; partial = sum g,
 *           sum g xhat) ; occd_bn_bwd_combine (partial -> packed[2C] fp32) ; [all-reduce a copy] ; occd_bn_bwd_finish
 *           (k1, k2, k3, gw = local sum g xhat, gb = local sum g) ; occd_bn_bwd_apply: out = g k1 + x k2 + k3 and,
 *           when out2 != NULL, out2 = g (the gradient of a residual that was added before the activation).
 * `partial` holds occd_bn_blocks() * 2 * ceil4(C) floats.
 * ------------------------------------------------------------------------ */
typedef struct occd_bn_args {
    const void* x;
    const void* gy;
    const void* y;
    const void* res;
    void* out;
    void* out2;
    const float* a;
    const float* b;
    const float* mean;
    const float* invstd;
    const float* k1;
    const float* k2;
    const float* k3;
    float* partial;
    int64_t rows;
    int64_t S;
    int32_t batch;
    int32_t C, cw;
    int32_t dtype, layout;
    int32_t x_cs, x_coff, gy_cs, gy_coff, y_cs, y_coff, res_cs, res_coff, out_cs, out_coff, out2_cs, out2_coff;
    int32_t act, res_first;
    float slope;
    int32_t nblk;
} occd_bn_args;
int occd_bn_blocks(const occd_bn_args* a);
int occd_bn_stats(const occd_bn_args* a, void* stream);
int occd_bn_stats_combine(const occd_bn_args* a, double* packed, void* stream);
int occd_bn_finish(const double* packed, int32_t C, float eps, float momentum, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                   float* a, float* b, void* stream);
int occd_bn_apply(const occd_bn_args* a, void* stream);
int occd_bn_bwd_reduce(const occd_bn_args* a, void* stream);
int occd_bn_bwd_combine(const float* partial, int32_t nblk, int32_t C, float* packed, void* stream);
int occd_bn_bwd_finish(const float* local, const float* total, int32_t C, const double* packed_fwd, const float* mean,
                       const float* invstd, const float* a, float* k1, float* k2, float* k3, float* gw, float* gb,
                       void* stream);
int occd_bn_bwd_apply(const occd_bn_args* a, void* stream);
/* launch-count reductions for LOCAL statistics: combine + finish in one launch (forward / backward), and the whole forward /
 * backward of a small NCHW layer (occd_bn_small_ok: layout 1, batch * S <= 8192, C >= 64) in one launch, one workgroup
 * per channel.                                                                                                       */
int occd_bn_stats_finish(const occd_bn_args* a, double* packed, float eps, float momentum, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                         float* mean, float* invstd, float* av, float* bv, void* stream);
int occd_bn_bwd_combine_finish(const float* partial, int32_t nblk, int32_t C, const double* packed_fwd, const float* mean,
                               const float* invstd, const float* a, float* k1, float* k2, float* k3, float* gw, float* gb,
                               void* stream);
int occd_bn_small_ok(const occd_bn_args* a);
int occd_bn_fwd_small(const occd_bn_args* a, double* packed, float eps, float momentum, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, int64_t* num_batches_tracked, float* mean, float* invstd,
                      float* av, float* bv, void* stream);
int occd_bn_bwd_small(const occd_bn_args* a, float* gw, float* gb, void* stream);
/* Round 5: the one-launch small layer with SYNCHRONISED statistics (SyncBatchNorm over the ranks of one node): workgroup c
 * exchanges channel c's packet with the peers' workgroups c inside the launch, through peer-mapped CHANNEL mailboxes
 * (occd_bn_xchg_mailbox_bytes(world, cmax) bytes each, created / opened with the occd_ipc_mailbox_* calls; one 64-byte
 * record of six self-validating {data : 32, sequence : 32} words per (slot, rank, channel); the fence-free protocol, the
 * determinism and the bounded wait of occd_ipc_allreduce).
 * mailboxes: HOST array of `world` device pointers, [rank] = own; C <= cmax.  Forward: `packed` receives the TOTALS over the
 * ranks [sum n mean, sum (M2 + n mean^2), sum n]; backward: packed_fwd = that vector, gw / gb stay this rank's sums.
 * Every rank must be able to schedule its workgroups while the peers' wait (one GPU per rank).  A peer's packet that does
 * not arrive within timeout_ms makes that channel's totals NaN (and sets *status), as in occd_ipc_allreduce.           */
int64_t occd_bn_xchg_mailbox_bytes(int32_t world, int32_t cmax);
int occd_bn_fwd_small_xchg(const occd_bn_args* a, double* packed, float eps, float momentum, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                           float* mean, float* invstd, float* av, float* bv, void* const* mailboxes, int32_t rank,
                           int32_t world, int32_t cmax, int32_t timeout_ms, int32_t* status, void* stream);
int occd_bn_bwd_small_xchg(const occd_bn_args* a, const double* packed_fwd, float* gw, float* gb, void* const* mailboxes,
                           int32_t rank, int32_t world, int32_t cmax, int32_t timeout_ms, int32_t* status, void* stream);

/* ------------------------------------------------------------------------ *
 * K2b / K8b: the same convolution forward (data gradient: the forward on dL/dy with flipped weights) and weight
 * gradient on the bf16 matrix pipe -- v_mfma_f32_32x32x16_bf16, fp32 accumulate, fp32 master weights -- for the bf16
 * training step (BASELINE configs[3]; reference call sites as for K2 / K8, plus the 3x3 convolutions of the 2-D decoder,
 * occdepth/models/unet2d.py:24-46, as X = 1 volumes of channels-last images).
 * `dtype` selects the storage type of the activation tensors (in, out, res1, res2 / x, gy): 0 = fp32 (converted to
 * bf16 while staging: "bf16 MFMA, fp32 storage"), 1 = bf16 (pointers are cast; *_cs / *_coff count elements).
 * occd_conv3d_bf16_fwd[_phases] take the OCCD_CONV_* modes below: those two and OCCD_CONV_BF16X3 (float32, 3-way bf16
 * split), OCCD_CONV_F16X2_HEAD (float32, two-term fp16 split, head geometry only, not _phases) and OCCD_CONV_F16X2 (float32,
 * two-term fp16 split, generic); see the packers of their weight images further down.
 * bias, dw and the workspace stay fp32.  `wpk` is the image of occd_pack_weights_bf16():
 *   wpk[tap][k16][nt][lane][j] (bf16),  value = W[cout = nt*32 + (lane & 31)][cin = k16*16 + (lane >> 5)*8 + j][tap].
 * act_in: NONE or RELU.  K8b stages voxel rows row-major in LDS and reads both MFMA operands with the gfx950
 * transposed LDS read (ds_read_b64_tr_b16); at most 28 taps.
 * ------------------------------------------------------------------------ */
int64_t occd_packed_weight_bf16_elems(int32_t cout, int32_t cin, int32_t taps);
int occd_pack_weights_bf16(const float* w, const float* scale, void* wpk,
                           int32_t cout, int32_t cin, int32_t kx, int32_t ky, int32_t kz,
                           int32_t layout, void* stream);
#define OCCD_CONV_F32 0        /* float32 tensors, converted to bf16 while staging */
#define OCCD_CONV_BF16 1       /* bfloat16 tensors */
#define OCCD_CONV_BF16X3 2     /* float32 tensors, 3-way bf16 split (image of occd_pack_weights_bf16x3) */
#define OCCD_CONV_F16X2_HEAD 3 /* float32 tensors, two-term fp16 split on K2s3h: the head geometry only */
#define OCCD_CONV_F16X2 4      /* float32 tensors, two-term fp16 split on the generic kernel (K2bh) */
int occd_conv3d_bf16_fwd(const occd_conv3d_args* a, int32_t dtype, void* stream);
/* the bf16-pipe twin of occd_conv3d_fwd_phases (same contract; dtype as above; with OCCD_CONV_BF16X3 also act_in = SIGMOID) */
int occd_conv3d_bf16_fwd_phases(const occd_conv3d_args* a, int32_t n, int32_t dtype, void* stream);
/* Pack a VIEW of a dense float32 weight tensor: element (co, ci, tap) of the packed operator is
 * w[co * s_co + ci * s_ci + tap_ofs[tap]] (tap_ofs: HOST array of ntaps <= 27 element offsets).  One launch instead of the
 * permute / index_select / contiguous chain autograd's data gradient needs for the transposed, flipped, tap-subset kernels
 * of its sub-pixel phases (torch.nn.grad.conv3d_input semantics; occdepth/models/OccDepth.py:535-537 backward).          */
int occd_pack_weights_gather(const float* w, const float* scale, float* wpk, int32_t cout, int32_t cin, int32_t ntaps,
                             int64_t s_co, int64_t s_ci, const int32_t* tap_ofs, void* stream);
int occd_pack_weights_bf16_gather(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                  int32_t ntaps, int64_t s_co, int64_t s_ci, const int32_t* tap_ofs, void* stream);
/* the same view as three images hi | mid | lo (3 x occd_packed_weight_bf16_elems elements): data-gradient operators of the 3-way
 * split (occd_conv3d_bf16_fwd, OCCD_CONV_BF16X3) */
int occd_pack_weights_bf16x3_gather(const float* w, const float* scale, void* wpk, int32_t cout, int32_t cin,
                                  int32_t ntaps, int64_t s_co, int64_t s_ci, const int32_t* tap_ofs, void* stream);
/* Opt-in experiment: OCCD_CONV_BF16X3 of occd_conv3d_bf16_fwd = float32 tensors, both operands split into three
 * bf16 terms (x = hi + mid + lo), six bf16 MFMAs per K step (hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid), fp32
 * accumulate: float32-level accuracy at 6/16 of the fp32-MFMA time.  Its weight image (3 x
 * occd_packed_weight_bf16_elems() elements: hi | mid | lo) comes from occd_pack_weights_bf16x3.                     */
int occd_pack_weights_bf16x3(const float* w, const float* scale, void* wpk,
                             int32_t cout, int32_t cin, int32_t kx, int32_t ky, int32_t kz,
                             int32_t layout, void* stream);
/* OCCD_CONV_F16X2_HEAD of occd_conv3d_bf16_fwd = float32 tensors, the two-term fp16 split (x = hi + 2^-11 lo', three fp16 MFMAs per K
 * step: lo_w * hi_x, hs_w * lo'_x, hi_w * hi_x), fp32 accumulate; the full-resolution head convolutions only (K2s3h: 3x3x3,
 * dilation = padding 1 / 2 / 3, <= 32 -> <= 32 channels on rows of >= 32 channels, Z a multiple of 32), anything else is
 * OCCD_EINVAL.  Finite activations with |x| >= 32760 overflow the fp16 operand and make the outputs they reach non-finite.
 * Its weight image (occd_packed_weight_f16x2_bytes() bytes, 16-byte aligned) comes from occd_pack_weights_f16x2: three fp16
 * images hi | hs | lo of w' = 2^k[co] w (layout of occd_pack_weights_bf16) and 32 * ceil(cout / 32) float epilogue factors.
 * Weights must be finite.  K2s3h keeps the hi and lo images in LDS for its lifetime and forms hs = hi 2^-11 in registers (the
 * stored hs image is read only by the ring form below; the image's format is unchanged).
 * occd_conv3d_head_set_lo: where K2s3h takes lo from -- 1 (the default) the resident LDS image; 0 the form before: hi | hs in
 * LDS, lo streamed from L2 through a register ring.  The outputs of both are bit-identical.  OCCD_HEAD_LO=0 in the environment
 * (read once) selects 0 as well; returns the previous setting; a value outside 0..1 selects 1.  (Added without a change of any
 * struct or prototype: no ABI bump.)
 * OCCD_CONV_F16X2 of occd_conv3d_bf16_fwd and occd_conv3d_bf16_fwd_phases = the same numerics and weight image on the generic kernel
 * (K2bh: any geometry OCCD_CONV_BF16X3 takes; act_in NONE or RELU only): only the hi and lo images are streamed, hs = hi 2^-11 is formed
 * in registers, the epilogue reads the factors of each phase's own image.  Same overflow contract as OCCD_CONV_F16X2_HEAD.               */
int64_t occd_packed_weight_f16x2_bytes(int32_t cout, int32_t cin, int32_t taps);
int occd_pack_weights_f16x2(const float* w, const float* scale, void* wpk,
                            int32_t cout, int32_t cin, int32_t kx, int32_t ky, int32_t kz,
                            int32_t layout, void* stream);
int32_t occd_conv3d_head_set_lo(int32_t form);
int64_t occd_conv3d_wgrad_bf16_workspace_floats(const occd_conv3d_wgrad_args* a, int32_t dtype);
int occd_conv3d_wgrad_bf16(const occd_conv3d_wgrad_args* a, int32_t dtype, void* stream);

/* SURVEY 8(f) row N1 (first step): the scene-completion losses of one training step as ONE pass over the
 * logits.  Everything occdepth/loss/ssc_loss.py:17-99 (geo_scal_loss, sem_scal_loss, CE_ssc_loss) and the inline
 * frustum-proportion loss of occdepth/models/OccDepth.py:487-521 compute is a function of these sums over voxels
 * (p = softmax over C of logits (B, C, S); t = target (B, S) uint8, 255 = unlabelled; map_occ != 0 applies the
 * cascade-head relabelling of OccDepth.py:413-415 to t first):
 *   stats[0 .. C)        P[c]  = sum_{t != 255} p_c            Q32 fixed point
 *   stats[C .. 2C)       N[c]  = sum_{t == c} p_c              Q32
 *   stats[2C .. 3C)      T[c]  = #{t == c}                     exact
 *   stats[3C]            M     = #{t != 255}                   exact
 *   stats[3C + 1]        sum_{t != 255} w_t * (-log p_t)       Q24   (w = weights, NULL = 1)
 *   stats[3C + 2]        sum_{t != 255} w_t                    Q24
 *   stats[3C + 3 + f*C + c]  sum_{masks[b, f, s] != 0} p_c     Q32   (masks (B, F, S) bytes; all voxels, labelled
 *                                                                     or not, as the reference)
 * Integer accumulation: results are independent of the order of the atomics (deterministic).  C <= 32.        */
int64_t occd_ssc_stats_len(int32_t C, int32_t F);
int occd_ssc_loss_stats_fwd(const float* logits, const uint8_t* target, const uint8_t* masks,
                            const float* weights, int64_t* stats, int64_t batch, int32_t C, int64_t S,
                            int32_t F, int32_t map_occ, void* stream);
/* grad (B, C, S) = d loss / d logits given gstats = d loss / d (the REAL-valued sums above, same layout; the
 * entries of the counts are ignored):  grad_c = p_c (g_c - sum_k p_k g_k) + [t != 255] gstats[3C+1] w_t (p_c - [c == t])
 * with g_c = [t != 255] (gP[c] + [t == c] gN[c]) + sum_{f : mask} gF[f][c].                                     */
int occd_ssc_loss_stats_bwd(const float* logits, const uint8_t* target, const uint8_t* masks,
                            const float* weights, const float* gstats, float* grad, int64_t batch, int32_t C,
                            int64_t S, int32_t F, int32_t map_occ, void* stream);
/* Round 5: the same three passes on logits (and gradients) that are NOT (B, C, S) planes -- element (b, c, s) at
 * b*s_b + c*s_c + s*s_v floats.  (s_c, s_v) = (S, 1) is the plane layout above; (1, cs) is the 3-D stack's own
 * channels-last voxel rows (cs % 4 == 0, 16-byte aligned base), read with 16-byte loads: the two 168 MB layout copies
 * of `ssc_logit` per training step (profiles/r04_train_step_bf16_aten_ops.txt) are gone.  bwd: grad has its own strides
 * (g_b, g_c, g_v); for channels-last grad rows the channels [C, g_pad) are written as zeros (g_pad % 4 == 0,
 * C <= g_pad <= g_v; 0 for the plane layout).                                                                       */
int occd_ssc_loss_stats_fwd_strided(const float* logits, const uint8_t* target, const uint8_t* masks,
                                    const float* weights, int64_t* stats, int64_t batch, int32_t C, int64_t S,
                                    int32_t F, int32_t map_occ, int64_t s_b, int64_t s_c, int64_t s_v, void* stream);
int occd_ssc_loss_stats_bwd_strided(const float* logits, const uint8_t* target, const uint8_t* masks,
                                    const float* weights, const float* gstats, float* grad, int64_t batch, int32_t C,
                                    int64_t S, int32_t F, int32_t map_occ, int64_t s_b, int64_t s_c, int64_t s_v,
                                    int64_t g_b, int64_t g_c, int64_t g_v, int32_t g_pad, void* stream);
int occd_ssc_confusion_strided(const float* logits, const uint8_t* labels, const uint8_t* target, int64_t* hist,
                               int64_t batch, int32_t C, int64_t S, int64_t s_b, int64_t s_c, int64_t s_v, void* stream);

/* the relation (context prior) loss, occdepth/loss/CRP_loss.py:4-24 -- BCEWithLogits with
 * pos_weight[r] = #negatives / #positives of relation r over the batch, mean over all B*R*M*N elements -- as ONE pass:
 *   loss = 1 / (R T) * sum_r ( pw_r * Spos_r + Sneg_r ),  T = B M N,
 *   stats[3 r + 0] = #{y = 1},  stats[3 r + 1] = sum_{y = 1} softplus(-x)  (Q24),  stats[3 r + 2] = sum_{y = 0} softplus(x)  (Q24)
 * (integer accumulation: deterministic).  logits: element (b, r, m, n) at b*l_b + r*l_r + m*l_m + n*l_n floats with
 * l_m == 1 or l_n == 1 (the HIP forward produces (R, B, N, M) rows, the autograd graph (B, R, M, N)); labels: the batch's
 * CP_mega_matrices, (B, R, N, M) contiguous, label_dtype 0 = uint8 (the dataloader's), 1 = float32.
 * grad: d loss / d logits = y ? -coef[2r] * sigmoid(-x) : coef[2r + 1] * sigmoid(x), written with the logits' strides;
 * coef (R, 2) device floats = g * (pw_r, 1) / (R T).                                                               */
int occd_relation_bce_stats(const float* logits, const void* labels, int32_t label_dtype, int64_t* stats,
                            int64_t batch, int32_t R, int64_t M, int64_t N, int64_t l_b, int64_t l_r, int64_t l_m,
                            int64_t l_n, void* stream);
int occd_relation_bce_grad(const float* logits, const void* labels, int32_t label_dtype, const float* coef,
                           float* grad, int64_t batch, int32_t R, int64_t M, int64_t N, int64_t l_b, int64_t l_r,
                           int64_t l_m, int64_t l_n, void* stream);

/* the depth-distribution loss of FLoSP-Depth, occdepth/loss/depth_loss.py:14-87, one thread per
 * prediction cell: nearest-resample the (Bn, srcH, srcW) metric depth map to cell x (h, w), smallest non-zero depth of
 * every cell x cell block, LID bin k = trunc((d - d_off) / d_step) (d_off = float32(d_bound[0] - d_bound[2])), target =
 * one-hot(k)[1:], BCE(prob, target) with both logs clamped at -100, summed over the D bins of every cell that has a
 * target.  prob: (Bn, D, h, w) probabilities, image stride p_b floats (a camera slice of (B, n_cams, D, h, w)).
 *   stats[0] = sum over measured cells (Q24 fixed point), stats[1] = #measured cells;  loss = stats[0] / max(1, stats[1]).
 * grad (Bn, D, h, w) dense = gscale[0] * (p - t) / max((1 - p) p, 1e-12) on measured cells, 0 elsewhere (ATen's
 * binary_cross_entropy_backward); gscale = device scalar g / max(1, #measured).                                   */
int occd_depth_bce_stats(const float* prob, const float* gt, int64_t* stats, int64_t Bn, int32_t D, int32_t h,
                         int32_t w, int32_t srcH, int32_t srcW, int32_t cell, int64_t p_b, float d_off, float d_step,
                         void* stream);
int occd_depth_bce_grad(const float* prob, const float* gt, const float* gscale, float* grad, int64_t Bn, int32_t D,
                        int32_t h, int32_t w, int32_t srcH, int32_t srcW, int32_t cell, int64_t p_b, float d_off,
                        float d_step, void* stream);

/* hist[t * C + pred] += 1 over voxels with t != 255 -- every counter
 * occdepth/loss/sscMetrics.py:70-204 (SSCMetrics.add_batch) keeps derives from this matrix.  pred is either
 * `labels` (B, S) uint8 or the arg-max over C of `logits` (B, C, S) (first maximum wins, as np.argmax in
 * OccDepth.py:523-526); exactly one of the two is non-NULL.  hist is NOT cleared (it accumulates).         */
int occd_ssc_confusion(const float* logits, const uint8_t* labels, const uint8_t* target, int64_t* hist,
                       int64_t batch, int32_t C, int64_t S, void* stream);

/* The same counts BY REGION in one pass over a (B, X, Y, Z) volume (voxel n = (x*Y + y)*Z + z): every labelled voxel is
 * counted into each of R <= OCCD_MAX_REGIONS regions it belongs to,
 *   hist[b * frame_stride + r*C*C + t*C + pred] += 1,
 * frame_stride = 0: all frames share one set of R matrices; frame_stride >= R*C*C: one set per frame.  hist accumulates.
 * A region is a half-open index box and a set of required flags, `need`: bit 0 = inside the camera field of view, bits
 * 1..3 = masks[0..2][b, n] != 0.  The descriptors travel by value with the launch (capture-safe: no device table, no
 * copy, no allocation).  The FOV flag is either the byte mask `fov` (B, S) or, when `fov` is NULL, computed from the
 * calibration exactly as occd_vox2pix computes fov[b, v, n, 0]: a voxel is inside when it is inside any view v whose bit
 * is set in view_mask (a horizontal image flip does not change the flag, so there is no ida).  Exactly one of the two
 * sources may be given.  pred as in occd_ssc_confusion: `labels` (B, S) or the arg-max (first maximum) of `logits` with
 * element (b, c, n) at b*s_b + c*s_c + n*s_v floats; channels-last rows (s_c = 1, s_v % 4 == 0, s_b % 4 == 0, 16-byte
 * aligned base) are read with 16-byte loads.  Voxels with t == 255, t >= C or pred >= C are dropped in every region.
 * OCCD_EINVAL before any launch: both or neither of logits / labels, R outside 1..8, an empty or out-of-grid box, a need
 * bit without its mask / FOV source, C outside 1..32, R*C*C*4 > 64 KiB (the workgroup's LDS counters), n_views outside
 * 1..4 or a view_mask that selects no view of them when the FOV is computed, frame_stride < 0 or in (0, R*C*C).      */
#define OCCD_MAX_REGIONS 8
typedef struct occd_confusion_region {
    int32_t x0, x1, y0, y1, z0, z1;   /* [x0, x1) x [y0, y1) x [z0, z1), inside the grid, not empty                   */
    uint32_t need;                    /* bit 0: FOV, bits 1..3: masks[0..2]                                         */
    int32_t reserved;
} occd_confusion_region;
typedef struct occd_confusion_regions_args {
    const float* logits;       /* or NULL                                                                           */
    const uint8_t* labels;     /* (B, S) or NULL                                                                    */
    const uint8_t* target;     /* (B, S), 255 = unlabelled                                                          */
    const uint8_t* masks[3];   /* (B, S) each, non-zero = member; NULL when unused                                  */
    const uint8_t* fov;        /* (B, S) explicit FOV mask, or NULL                                                 */
    const double* cam_E;       /* (B, V, 4, 4) device float64, or NULL                                              */
    const double* cam_k;       /* (B, V, 3, 3) device float64, or NULL                                              */
    int64_t* hist;
    int64_t s_b, s_c, s_v;     /* logits strides in floats                                                          */
    int64_t frame_stride;      /* 0 or >= R*C*C                                                                     */
    double vox_origin[3];      /* rounded to float32 as vox2world does                                              */
    double voxel_size;
    int32_t batch, C, X, Y, Z, R;
    int32_t n_views, view_mask, img_w, img_h;
    occd_confusion_region regions[OCCD_MAX_REGIONS];
} occd_confusion_regions_args;
int occd_ssc_confusion_regions(const occd_confusion_regions_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * Training targets of the SemanticKITTI dataloader, built on the GPU (csrc/targets.hip).  All three are bit-exact
 * restatements of the reference's numpy functions and capture-safe: calibration is read from device memory, the
 * counters are zeroed by a fill kernel, nothing is allocated and nothing synchronises.
 *
 * occd_frustum_targets: compute_local_frustums (occdepth/data/utils/helpers.py:183-260, dataset "kitti") over the
 * voxel -> pixel projection of occd_project_voxels (pattern point 0), for V = 1 or 2 views.  Voxel n = (x*Y + y)*Z + z
 * lies in frustum f = j*s + i of a view when  (i/s)*W <= pix_x < ((i+1)/s)*W,  (j/s)*H <= pix_y < ((j+1)/s)*H  and
 * cam_z > 0, all compared in float64 as helpers.py:172-180,216-224 does.
 *   masks[b, f, n] = target[b, n] != 255 && (n in frustum f of any view)                    (B, F, N) uint8, F = s*s
 *   dists[b, f, c] = #{n : masks[b, f, n] && target[b, n] == c}, c < n_classes               (B, F, C) float32
 * Labels in [n_classes, 255) enter the masks but no count.  Requires 1 <= s <= 16 and F * n_classes <= 4096. */
typedef struct occd_frustum_args {
    const double* cam_E;       /* (B, V, 4, 4) device float64, row major (lidar -> camera)                   */
    const double* cam_k;       /* (B, V, 3, 3) device float64 (fx, fy, cx, cy are rounded to float32)        */
    const uint8_t* target;     /* (B, N) labels, 255 = unlabelled                                            */
    uint8_t* masks;            /* (B, F, N)                                                                  */
    float* dists;              /* (B, F, C); used as uint32 counters until the last launch converts them     */
    double vox_origin[3];
    double voxel_size;
    int32_t batch, n_views, X, Y, Z;
    int32_t img_w, img_h, frustum_size, n_classes;
} occd_frustum_args;
int occd_frustum_targets(const occd_frustum_args* a, void* stream);

/* _downsample_label (occdepth/data/NYU/preprocess.py:102-143, used by data/semantic_kitti/preprocess.py for the
 * 1:8 labels): every ds^3 block of `in` (B, X, Y, Z) uint8 -> one label of `out` (B, X/ds, Y/ds, Z/ds):
 * zero = #0 + #255;  zero > 0.95 * ds^3 ? (#0 > #255 ? 0 : 255) : the most frequent label in 1..254 (smallest on a tie).
 * X, Y and Z must be multiples of ds. */
int occd_downsample_label(const uint8_t* in, uint8_t* out, int32_t batch, int32_t X, int32_t Y, int32_t Z, int32_t ds,
                          void* stream);

/* compute_CP_mega_matrix (occdepth/data/utils/helpers.py:6-91): `coarse` (B, X, Y, Z) uint8 labels ->
 * out (B, R, N, M) uint8, N = X*Y*Z, M = (X/2)(Y/2)(Z/2) mega voxels (index (xx*(Y/2) + yy)*(Z/2) + zz, children
 * (2xx+dx, 2yy+dy, 2zz+dz)); R = 4 (non-non same, non-non diff, empty-empty, nonempty-empty) or, with `binary`,
 * R = 2 (diff, same).  Entry (r, n, m) depends on label[n] and the set of non-255 child labels of m only; rows
 * labelled 255 are zero.  Every byte of `out` is written. */
int occd_cp_mega_matrix(const uint8_t* coarse, uint8_t* out, int32_t batch, int32_t X, int32_t Y, int32_t Z,
                        int32_t binary, void* stream);

/* The label decode of the reference's SemanticKITTI preprocessing pass (occdepth/data/semantic_kitti/preprocess.py:76-84
 * over io_data.py:10-22,122-134,175-195) and the `.occluded` volume of kitti_dataset.py:312-313, for a whole batch of raw
 * voxel files:
 *   raw           (B, N) uint16, the `.label` file: N = X*Y*Z voxels in (X, Y, Z) row-major order; 2-byte aligned is enough
 *   invalid_bits  (B, N/8) uint8, the `.invalid` file: voxel 8k + j is bit 7 - j of byte k (io_data.unpack, MSB first)
 *   occluded_bits optional, the `.occluded` file, packed the same way; given exactly when `occluded` is
 *   lut           uint8[lut_len], 1 <= lut_len <= 4096 (io_data.get_remap_lut: 359 entries)
 *   target[b, n]   = invalid bit set or raw >= lut_len ? 255 : lut[raw[b, n]]                    (B, N) uint8, 8-byte aligned
 *   occluded[b, n] = the occluded bit, 0 or 1                                                   (B, N) uint8, 8-byte aligned
 *   *out_of_range  = #{(b, n) : raw[b, n] >= lut_len} (the reference raises IndexError there); device int32, set by every
 *                    call (a fill kernel, not a memset node), never read back here.
 * N must be a multiple of 8.  Nothing is allocated and nothing synchronises: capture-safe. */
int occd_kitti_labels(const uint16_t* raw, const uint8_t* invalid_bits, const uint8_t* occluded_bits, const uint8_t* lut,
                      int32_t lut_len, uint8_t* target, uint8_t* occluded, int32_t* out_of_range, int32_t batch, int64_t N,
                      void* stream);

/* ------------------------------------------------------------------------ *
 * Global gradient-norm clipping fused with the AdamW update (csrc/optim.hip): the "grad-clip 35 -> AdamW" stage of the
 * reference's training step (`gradient_clip_val: 35` in every yaml under occdepth/config/, handed to the Trainer at
 * occdepth/scripts/train.py:188,204 = torch.nn.utils.clip_grad_norm_(params, 35) before torch.optim.AdamW.step()).
 * Multi-tensor, float32 only: the kernels walk a table of chunk descriptors, one workgroup per descriptor, so any number
 * of parameter tensors costs three launches.  A tensor of n elements contributes max(1, ceil(n / OCCD_OPTIM_CHUNK))
 * consecutive descriptors (offset 0, CHUNK, 2 CHUNK, ...); tensors may start at any 4-byte alignment.
 *
 * The table is read BY THE KERNELS and must stay valid and unchanged for as long as a launch -- or a captured graph
 * that holds one -- can run: device memory, or pinned host memory the device can address (hipHostMalloc; the kernels
 * then fetch one 64-byte descriptor per workgroup across the bus, and no copy node enters a capture).  Pageable host
 * memory is rejected.
 *
 *   occd_grad_sumsq   2 launches: per-chunk sum of squares of the gradients, accumulated in float64 into
 *                     partials[chunk]; then one workgroup adds the partials in a fixed order and writes
 *                       norm_out[0] = total_norm = sqrt(sum)                         (float32)
 *                       norm_out[1] = clip_coef  = min(1, max_norm / (total_norm + 1e-6)), NaN if the norm is NaN, 0 if Inf
 *                     No atomics, no counters, nothing to zero: bit-identical from run to run.
 *   occd_clip_adamw   the same two launches -- the workgroup of every tensor's first chunk also advances that tensor's
 *                     `step` by one -- and the update, one read of p, g, m, v and one write of p, m, v per element:
 *                       g' = clip_coef g (in registers: the gradient in memory stays unscaled)
 *                       p *= 1 - lr wd;  m = m + (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2
 *                       p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 *                     torch.optim.AdamW's arithmetic in its order, evaluated in float64 and rounded once per stored value.
 * lr is read from the device scalar `lr_dev` when it is not NULL (a scheduler's change reaches a captured launch),
 * else from `lr`. */
#define OCCD_OPTIM_CHUNK 8192
typedef struct occd_optim_chunk {      /* 64 bytes: one fetch per workgroup                                          */
    float* p;                          /* parameter tensor (first element)                                           */
    const float* g;                    /* its gradient                                                               */
    float* m;                          /* exp_avg                                                                    */
    float* v;                          /* exp_avg_sq                                                                 */
    float* step;                       /* the parameter's step counter, device float32 scalar                        */
    int64_t offset;                    /* first element of this chunk inside the tensor                              */
    int32_t count;                     /* elements of this chunk, 0 .. OCCD_OPTIM_CHUNK (0: an empty tensor)         */
    int32_t reserved0;
    float* acc;                        /* gradient accumulator of a window of micro-batches (occd_accum_clip_adamw), or NULL */
} occd_optim_chunk;

typedef struct occd_clip_adamw_args {
    const occd_optim_chunk* chunks;    /* n_chunks descriptors, see above                                            */
    double* partials;                  /* n_chunks float64, device workspace                                         */
    float* norm_out;                   /* 2 device floats: total_norm, clip_coef                                     */
    const float* lr_dev;               /* device scalar learning rate, or NULL                                       */
    int64_t n_chunks;
    int64_t n_elems;                   /* elements over all chunks (profiling only)                                  */
    double lr, beta1, beta2, eps, weight_decay;
    double max_norm;                   /* > 0                                                                        */
} occd_clip_adamw_args;
int occd_grad_sumsq(const occd_clip_adamw_args* a, void* stream);
int occd_clip_adamw(const occd_clip_adamw_args* a, void* stream);

/* Gradient accumulation over a window of N micro-batches, fused into the clip + AdamW above (what
 * `Trainer(accumulate_grad_batches=N)` does under automatic optimisation: backward of loss / N into p.grad N times, then
 * clip_grad_norm_ and AdamW.step() once).  Called once per micro-batch with the micro-batch's position in its window:
 *
 *   every micro-batch   1 launch, one workgroup per descriptor: acc = scale g when `first` (an overwrite: accumulators are
 *                       never zeroed and never read before they are written), else acc = acc + scale g; float64
 *                       arithmetic, each stored value rounded once; 4 + 8 bytes per element (4 + 4 when `first`).
 *   when `last`         the same workgroups also leave the sum of squares of the acc values they stored in partials[chunk]
 *                       (max_norm > 0 only) and advance every tensor's `step`; then the norm finalise of occd_grad_sumsq
 *                       (max_norm > 0 only) and the update of occd_clip_adamw with acc in place of g.  max_norm <= 0: no
 *                       clipping -- no norm is computed, norm_out is not touched and the coefficient is exactly 1.
 *   when not `last`     p, m, v, step and norm_out keep their bits.
 *
 * The position comes from `flags_dev` (two device int32: first, last) when it is not NULL -- then all three launches are
 * always enqueued and leave early by themselves, which is what a captured graph needs: one capture serves every position
 * and the caller rewrites the two ints before a replay -- else from the host ints `first` / `last`, and the launches a
 * non-closing micro-batch does not need are not made.  Every descriptor's `acc` must be set, n elements like its tensor,
 * with the same offset to a 16-byte boundary as `p`; `g` may sit at any 4-byte alignment and is never written.  No
 * atomics, nothing to zero, bit-identical from run to run; with scale = 1 and first = last = 1 the results are those of
 * occd_clip_adamw. */
typedef struct occd_accum_adamw_args {
    const occd_optim_chunk* chunks;    /* n_chunks descriptors with `acc` set                                        */
    double* partials;                  /* n_chunks float64, device workspace (max_norm > 0)                          */
    float* norm_out;                   /* 2 device floats: total_norm, clip_coef of the last closed window (max_norm > 0) */
    const float* lr_dev;               /* device scalar learning rate, or NULL                                       */
    const int32_t* flags_dev;          /* 2 device ints {first, last}, or NULL: the host ints below                  */
    int64_t n_chunks;
    int64_t n_elems;                   /* elements over all chunks (profiling only)                                  */
    double lr, beta1, beta2, eps, weight_decay;
    double max_norm;                   /* <= 0: no clipping                                                          */
    double scale;                      /* 1 / N, in (0, 1]                                                           */
    int32_t first, last;               /* read when flags_dev is NULL                                                */
} occd_accum_adamw_args;
int occd_accum_clip_adamw(const occd_accum_adamw_args* a, void* stream);

/* ------------------------------------------------------------------------ *
 * Small-message all-reduce over peer-mapped device memory (round 5; csrc/ipc_allreduce.hip): the latency-optimal form
 * of SyncBatchNorm's per-layer exchange of (2C + 1) statistics -- `Trainer(sync_batchnorm=True)`,
 * occdepth/scripts/train.py:176-206 -- one kernel per call, no library, deterministic (rows summed in rank order).
 * Set-up (once per process group, host side): every rank creates a mailbox of occd_ipc_mailbox_bytes(world, max_bytes)
 * bytes (fine-grained device memory, zeroed) and its 64-byte IPC handle, the handles are exchanged by any means
 * (torch.distributed object collectives), every rank opens its peers' handles.  Call: all ranks issue the same sequence of
 * occd_ipc_allreduce calls (dtype 0 float32 / 1 float64, count * elem <= max_bytes) on a stream; `mailboxes` is a HOST
 * array of `world` device pointers, [rank] = the rank's own mailbox; the per-call sequence number lives in the mailbox and
 * is advanced by the kernel, so a captured launch replays correctly.  Wire format: every 32-bit half of the payload in its
 * own 8-byte word {data, sequence}, one system-scope atomic store / load each -- no fence anywhere.  The wait is bounded by timeout_ms (<= 0: unbounded):
 * on expiry the kernel sets *status = 1 (device int, optional) and writes NaN into the elements of `out` whose wait gave up
 * (never a partial sum: a lost peer poisons the step's loss instead of silently skewing it).                          */
int64_t occd_ipc_mailbox_bytes(int32_t world, int64_t max_bytes);
int occd_ipc_mailbox_create(int64_t bytes, void** mailbox, void* handle64);
int occd_ipc_mailbox_open(const void* handle64, void** peer);
int occd_ipc_mailbox_close(void* peer);
int occd_ipc_mailbox_free(void* mailbox);
int occd_ipc_allreduce(const void* in, void* out, int64_t count, int32_t dtype, void* const* mailboxes, int32_t rank,
                       int32_t world, int64_t max_bytes, int32_t timeout_ms, int32_t* status, void* stream);

/* ------------------------------------------------------------------------ *
 * Temporal fusion of class probabilities over a sequence (csrc/fuse.hip).  Additive (OCCD_ABI_VERSION note).  No
 * atomics, no allocation, no host sync (capture-safe); every output byte depends on the inputs alone.
 *
 * occd_fuse_store: one frame's logits (one batch item), element (c, n) at c*s_c + n*s_v floats, -> softmax rows,
 * rows[n*pitch + c], voxel n = (x*Y + y)*Z + z.  Layouts: planes (s_v == 1, s_c >= S) and channels-last rows (s_c == 1,
 * s_v >= C).  Channels-last rows with s_v % 4 == 0, s_v >= round4(C) and a 16-byte aligned base are read in 16-byte pieces
 * (the floats [C, round4(C)) of a row are read and dropped); any other channels-last rows go through
 * occd_softmax_channels.  The channels [C, round4(C)) of every output row are written as zeros (the 16-byte path and the
 * planes: the whole pad [C, pitch)).  `rows` 16-byte aligned.  OCCD_EINVAL before any launch: a NULL pointer, C outside
 * 1..32, S outside 1..2^28, pitch < round4(C) or pitch % 4 != 0, any other stride pair.
 *
 * occd_fuse_frames, one launch: for every voxel (i, j, l) of the X x Y x Z grid and every source k < K (float32; the
 * three sums of a component are fused multiply-adds, b first, then the z, y and x terms)
 *   s   = A_k (i + 1/2, j + 1/2, l + 1/2) + b_k        affine[k] = A_k row-major | b_k, grid units
 *   idx = floor(s) per component;  ok = 0 <= idx < (X, Y, Z) and (masks[k] == NULL or masks[k][idx] != 0)
 *   acc[c] += weights[k] * rows[k][idx][c],  wsum += weights[k],  n += 1        where ok, k ascending
 * (nearest voxel, no interpolation; a non-finite s is not ok).  labels[n] = argmax_c acc[c], the lowest class on a tie;
 * n_obs[n] = n; prob (when not NULL): rows of `pitch` floats, prob[n][c] = acc[c] / wsum for c < round4(C), channels
 * past that are left alone.  A voxel with n == 0 gets label 0, n_obs 0 and a zero prob row.  Rows and prob 16-byte
 * aligned; the channels [C, round4(C)) of the source rows must be finite (occd_fuse_store writes zeros).
 * OCCD_EINVAL before any launch: a NULL argument / labels / n_obs / rows[k < K], C outside 1..32, K outside
 * 1..OCCD_FUSE_MAX_SOURCES, a non-positive dim, X Y Z > 2^28, pitch < round4(C) (so also pitch < C) or pitch % 4 != 0.
 * ------------------------------------------------------------------------ */
#define OCCD_FUSE_MAX_SOURCES 8
typedef struct OccdFuseArgs {
    const float* rows[OCCD_FUSE_MAX_SOURCES];      /* (X Y Z, pitch) probability rows of source k; k = 0: the current frame */
    const uint8_t* masks[OCCD_FUSE_MAX_SOURCES];   /* (X Y Z) bytes of source k, 0 = does not contribute, or NULL          */
    float weights[OCCD_FUSE_MAX_SOURCES];
    float affine[OCCD_FUSE_MAX_SOURCES][12];       /* target voxel centre -> source grid coordinates                       */
    uint8_t* labels;                               /* (X Y Z)                                                              */
    uint8_t* n_obs;                                /* (X Y Z) sources that contributed                                     */
    float* prob;                                   /* (X Y Z, pitch), or NULL                                              */
    int32_t X, Y, Z;
    int32_t C, K, pitch;
} OccdFuseArgs;
int occd_fuse_store(const float* logits, float* rows, int64_t S, int32_t C, int64_t s_c, int64_t s_v, int32_t pitch,
                    void* stream);
int occd_fuse_frames(const OccdFuseArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K30: the sequence-level semantic map (csrc/semantic_map.hip).  Additive (OCCD_ABI_VERSION note).  Every frame's labelled
 * voxels vote into one sparse world-frame voxel map; extraction decides every voxel by its votes.  No atomics, no
 * allocation, no host sync; every output byte depends on the inputs alone.
 *
 * World lattice: the map's voxel size is the frame grid's voxel size v; world voxel (I, J, L), signed, has its centre at
 * ((I + 1/2) v, (J + 1/2) v, (L + 1/2) v) metres in the world frame of the poses (4 x 4 sensor -> world).
 * Bricks: OCCD_MAP_BRICK^3 = 4096 voxels; brick key = floor((I, J, L) / 16) (negative coordinates floor).  The pool
 * `votes` holds `capacity` bricks; brick `slot` is 4096 rows of `pitch` unsigned 16-bit counters, row (i*16 + j)*16 + l
 * for the brick-local voxel (i, j, l), counter c of a row = the votes for class c.  pitch >= C and pitch % 4 == 0 (rows
 * are read in 8-byte pieces; `votes` 8-byte aligned): 8192 * pitch bytes per brick, 163840 at C = 20.  Counters saturate
 * at 65535.
 *
 * occd_map_integrate, one launch per frame, one workgroup per table row (= brick).  Row r of `table` is 16 int32:
 *   slot | key[3] | Aq[9] row-major | cq[3]
 * with Aq = rint(R^T 2^16) and cq = rint(c_k 2^16), c_k = (R^T ((16 k + 1/2) v - t) - o) / v for the pose [R|t], the grid
 * origin o (metres, sensor frame) and the key k, composed by the host in float64 (|c_k| < 2^14).  For the brick-local voxel
 * (i, j, l), in int32 only (wrapping):
 *   gq[r] = Aq[r][0] i + Aq[r][1] j + Aq[r][2] l + cq[r];   idx[r] = gq[r] >> 16   (arithmetic shift = floor)
 * and the voxel's counter `label` is incremented iff 0 <= idx < (X, Y, Z), (mask == NULL or mask[n] != 0) and label < C,
 * with n = (idx0 Y + idx1) Z + idx2 and label = labels[n] read as 1 or 2 bytes (label_bytes).  So 255 never votes.  A
 * row whose slot is outside [0, capacity) is skipped.  The slots of one launch must be distinct (one owner per counter).
 *
 * Extraction: label = argmax_c votes[c], the lowest class on a tie; n_obs = sum_c votes[c].  Row r of the extraction
 * `table` is 4 int32: slot | key[3]; a slot outside [0, capacity) is a brick that is not in the map.
 *   occd_map_brick_labels: dense[r][4096] = label, 255 where n_obs == 0 or the brick is not in the map.
 *   occd_map_count:   counts[r] = number of kept voxels of brick r: n_obs >= min_obs (and >= 1), label != 0 unless
 *                     include_empty.
 *   occd_map_extract: the kept voxels of brick r, in (i, j, l) row-major order, go to the entries offsets[r] ... of
 *                     coords (3 int32 each: 16 key + (i, j, l)), labels (uint8) and n_obs (uint16, the sum saturated at
 *                     65535).  offsets = the exclusive prefix sum of counts (int64).  Wave ballots and an LDS hand-off
 *                     order the writes: bit-identical from run to run.
 * `table_host`, when not NULL, is the same table in host memory: its slots are checked before the launch (integrate: a
 * slot outside [0, capacity); extraction: a slot >= capacity).  OCCD_EINVAL before any launch: a NULL argument or a NULL
 * votes / table / labels / output pointer, C outside 1..32, a non-positive dim, X Y Z > 2^28, n_bricks <= 0, capacity <= 0,
 * such a slot in table_host, label_bytes not 1 or 2, pitch < C or pitch % 4 != 0, min_obs < 0, n_out <= 0 (extract).
 * ------------------------------------------------------------------------ */
#define OCCD_MAP_BRICK 16
typedef struct OccdMapFrameArgs {
    uint16_t* votes;               /* (capacity, 4096, pitch) vote counters                                          */
    const int32_t* table;          /* (n_bricks, 16) device                                                          */
    const int32_t* table_host;     /* the same rows in host memory, or NULL                                          */
    const void* labels;            /* (X Y Z) labels of the frame, label_bytes each                                  */
    const uint8_t* mask;           /* (X Y Z) bytes, 0 = does not vote, or NULL                                      */
    int32_t n_bricks, capacity;
    int32_t X, Y, Z;
    int32_t C, pitch, label_bytes;
} OccdMapFrameArgs;
typedef struct OccdMapExtractArgs {
    const uint16_t* votes;         /* (capacity, 4096, pitch)                                                        */
    const int32_t* table;          /* (n_bricks, 4) device                                                           */
    const int32_t* table_host;     /* the same rows in host memory, or NULL                                          */
    uint8_t* dense;                /* occd_map_brick_labels: (n_bricks, 4096)                                        */
    int32_t* counts;               /* occd_map_count: (n_bricks)                                                     */
    const int64_t* offsets;        /* occd_map_extract: (n_bricks) exclusive prefix sum of counts                    */
    int32_t* coords;               /* occd_map_extract: (N, 3)                                                       */
    uint8_t* labels;               /* occd_map_extract: (N)                                                          */
    uint16_t* n_obs;               /* occd_map_extract: (N)                                                          */
    int64_t n_out;                 /* occd_map_extract: N = the sum of counts; no entry at or past it is written     */
    int32_t n_bricks, capacity;
    int32_t C, pitch;
    int32_t min_obs, include_empty;
} OccdMapExtractArgs;
int occd_map_integrate(const OccdMapFrameArgs* a, void* stream);
int occd_map_brick_labels(const OccdMapExtractArgs* a, void* stream);
int occd_map_count(const OccdMapExtractArgs* a, void* stream);
int occd_map_extract(const OccdMapExtractArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K32: read the sequence map back into a frame (occd_map_sample, csrc/semantic_map.hip).  Additive (OCCD_ABI_VERSION
 * note).  One launch per frame, one thread per frame voxel (z fastest): every voxel of the frame's (X, Y, Z) grid looks
 * up the world voxel its centre falls into and decides it by the votes the whole sequence left there.  The pool is only
 * read.  No atomics, no allocation, no host sync (capture-safe); every output byte depends on the inputs alone.
 *
 * Window: the inclusive brick-key box key_min .. key_max of the frame's candidate bricks (the brick range of the grid's
 * eight corners in world voxels, one voxel wider on every side); grid = key_max - key_min + 1 bricks, W0 = 16 key_min.
 * cells[(cx gy + cy) gz + cz] is the row in `table` of the brick at that cell, or negative where the map has no such brick.
 * `table` has integrate's layout, 16 int32 per row: slot | key[3] | Aq[9] | cq[3] (Aq, cq of THIS frame's pose).
 *
 * Geometry, int32 fixed point with 16 fractional bits (unsigned wrapping arithmetic; the host keeps |wq| < 2^31: it
 * refuses X + Y + Z >= 2^14 and |d| >= 2^14).  For the frame voxel g = (x, y, z), n = (x Y + y) Z + z:
 *   wq[r] = Bq[r][0] x + Bq[r][1] y + Bq[r][2] z + dq[r];   idx[r] = wq[r] >> 16   (arithmetic shift = floor)
 * with Bq = rint(R 2^16), dq = rint(d 2^16), d = R (1/2 + o / v) + t / v - W0 composed by the host in float64: idx is the
 * world voxel relative to W0.  cell = idx >> 4, local = idx & 15.  The brick is ABSENT when cell is outside grid, the
 * cell's row is outside [0, n_bricks) or that row's slot is outside [0, capacity); otherwise the voxel's counters are
 * the row (local0 * 16 + local1) * 16 + local2 of brick `slot`, read in 8-byte pieces.
 *
 * Decision per voxel.  flags & OCCD_MAP_SAMPLE_EXCLUDE_SELF takes this frame's own vote out: with the row's Aq | cq the
 * frame voxel n' that occd_map_integrate maps this world voxel to is computed (same formula, same wrapping), and the
 * counter own[n'] counts one less iff n' is inside (X, Y, Z), (own_mask == NULL or own_mask[n'] != 0), own[n'] < C, and
 * the counter is neither 0 nor 65535 (a saturated counter has forgotten how many votes it dropped and is not retracted).
 * n' need not be n: the two nearest-voxel maps are not inverses.  Then n_obs = the sum of the counters, label = their
 * arg-max, the lowest class on a tie.  flags & OCCD_MAP_SAMPLE_KEEP_OWN: if own[n] < C and its counter equals the
 * maximum and the maximum is > 0, label = own[n].  Outputs:
 *   labels[n] = label where n_obs >= max(min_obs, 1); elsewhere own[n] (a value >= 255 becomes 255) when own is given,
 *               else 255.  An absent brick has n_obs = 0.
 *   n_obs[n]  = the sum saturated at 65535, always written.
 * own is read as 1 or 2 bytes per voxel (label_bytes), as in occd_map_integrate.
 * OCCD_EINVAL before any launch: a NULL argument, NULL votes / table / cells / labels / n_obs, C outside 1..32, pitch < C
 * or pitch % 4 != 0 or votes not 8-byte aligned, non-positive dims, grid, n_bricks or capacity, X Y Z > 2^28,
 * gx gy gz > 2^27, a flag without own or an unknown flag, min_obs < 0, label_bytes not 1 or 2, a slot >= capacity in
 * table_host (a negative one is a brick that is not in the map).
 * ------------------------------------------------------------------------ */
#define OCCD_MAP_SAMPLE_EXCLUDE_SELF 1
#define OCCD_MAP_SAMPLE_KEEP_OWN 2
typedef struct OccdMapSampleArgs {
    const uint16_t* votes;         /* (capacity, 4096, pitch) vote counters, read only                               */
    const int32_t* table;          /* (n_bricks, 16) device                                                          */
    const int32_t* table_host;     /* the same rows in host memory, or NULL                                          */
    const int32_t* cells;          /* (gx, gy, gz) device: row of the brick, negative = absent                       */
    const void* own;               /* (X Y Z) labels of the frame itself, label_bytes each, or NULL                  */
    const uint8_t* own_mask;       /* (X Y Z) bytes, the mask the frame voted with, or NULL                          */
    uint8_t* labels;               /* (X Y Z) out                                                                    */
    uint16_t* n_obs;               /* (X Y Z) out                                                                    */
    int32_t n_bricks, capacity;
    int32_t X, Y, Z;
    int32_t gx, gy, gz;
    int32_t C, pitch, label_bytes;
    int32_t min_obs, flags;
    int32_t Bq[9], dq[3];          /* row-major rint(R 2^16), rint(d 2^16)                                           */
} OccdMapSampleArgs;
int occd_map_sample(const OccdMapSampleArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K33: the sum of two sets of bricks (occd_map_merge, csrc/semantic_map.hip).  Additive (OCCD_ABI_VERSION note).  Votes
 * are counters and commute: the map of a set of frames is the counter-wise saturating sum of the maps of any partition
 * of the set, and min(a + b + c, 65535) on non-negative counters depends on neither order nor grouping.
 *
 * `votes` is the destination pool of `capacity` bricks, `src` holds `src_capacity` bricks in the same layout (4096 rows
 * of `pitch` counters each: another map's pool, or a staging buffer of received rows); both 16-byte aligned, so every
 * brick and every 16-byte piece of one (512 * pitch per brick) is.  Row r of `table` is 2 int32: destination slot |
 * source row.  For every table row and every counter c of the brick, the padding counters included:
 *   votes[slot][c] = min(votes[slot][c] + src[row][c], 65535)
 * A table row whose slot is outside [0, capacity) or whose source row is outside [0, src_capacity) is skipped.  The
 * slots of one launch must be distinct, and `src` must not overlap the destination bricks (one owner per counter: no
 * atomics, the bytes written do not depend on the schedule).  One launch of n x split workgroups: a brick is cut into
 * `split` equal runs of pieces (1, 2, 4 or 8; 0 = the library's choice).  `table_host`, when not NULL, is the same
 * table in host memory: a row of it that the kernel would skip is refused instead.
 * n == 0 returns OCCD_OK without a launch.  OCCD_EINVAL before any launch: a NULL argument or NULL votes / src / table,
 * n < 0, capacity or src_capacity <= 0, pitch outside 4..32 or pitch % 4 != 0, votes or src not 16-byte aligned, a split
 * other than 0, 1, 2, 4, 8, such a row in table_host.
 * ------------------------------------------------------------------------ */
typedef struct OccdMapMergeArgs {
    uint16_t* votes;               /* (capacity, 4096, pitch) destination counters                                   */
    const uint16_t* src;           /* (src_capacity, 4096, pitch) source counters, read only                         */
    const int32_t* table;          /* (n, 2) device: destination slot | source row                                   */
    const int32_t* table_host;     /* the same rows in host memory, or NULL                                          */
    int32_t n, capacity, src_capacity;
    int32_t pitch, split;
} OccdMapMergeArgs;
int occd_map_merge(const OccdMapMergeArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K31: render the sequence map (csrc/map_render.hip).  Additive (OCCD_ABI_VERSION note).  One ray per pixel through the
 * sparse brick map, two levels: a directory `cells` of 16^3-voxel bricks over a window of (gx, gy, gz) bricks, and one
 * 4096-byte row of labels per brick.  One launch for n_views x H x W pixels, one thread per pixel, a wave per 8 x 8
 * pixel tile.  No atomics, no allocation, no host sync (capture-safe).
 *
 * Window: the box [0, 16 gx] x [0, 16 gy] x [0, 16 gz] in voxels; `views` are OccdRenderViews in these window voxel
 * units.  cells[(cx gy + cy) gz + cz] is the row of the brick at that cell; negative (or >= n_rows): the brick is absent.  Voxel
 * (x, y, z) of a present brick reads labels[row][((x & 15) 16 + (y & 15)) 16 + (z & 15)] (and target likewise).
 *
 * Contract: for t_max = +inf every pixel's (voxel, face, t, colour) equals, bit for bit, what occd_render_voxels gives
 * for the same view on the dense (16 gx, 16 gy, 16 gz) uint8 volume of the same labels in which every voxel of an absent
 * brick is 255 (target 255), without fov; hit = row * 4096 + the brick-local index of that voxel.  For a finite t_max
 * every hit of depth > t_max is a miss.  The ray set-up, the visibility rule and the colour rule are those of
 * occd_render_voxels above; every boundary time is m_a(i) = ((float)(i + (dir_a > 0)) - origin_a) * (1 / dir_a).
 * Inside a present brick the walk steps voxel by voxel.  An absent brick is left in one step: with last_a the brick's
 * last voxel index along each moving axis and M_a = m_a(last_a), the exit axis a has the smallest (M_a, a) (x before y
 * before z on ties); the ray ends when M_a > t_max or M_a is not below +inf; on every other moving axis b the index
 * becomes the first one whose crossing does not precede (M_a, a) in the voxel walk's merge order (m_b <= M_a for b < a,
 * m_b < M_a for b > a), found from the estimate floor(origin_b + dir_b M_a) clamped into the brick by single steps against
 * that predicate; then index_a = last_a + sign(dir_a), face = a, t = M_a.  The crossing times of an axis are monotone
 * in the index, so the voxel walk is a merge of three sorted sequences and the skip lands on a point of that merge.
 * flags bit 0: absent bricks are walked voxel by voxel (without label loads) instead -- same result, for A/B runs.
 * At most 16 (gx + gy + gz) + 3 iterations per ray (never reached: each moves at least one index one way).
 * OCCD_EINVAL without a launch: NULL labels / cells / views / palette / rgb, gx, gy or gz outside 1..65536,
 * gx gy gz > 2^27, n_rows <= 0, non-positive H or W, n_views outside 1..OCCD_RENDER_MAX_VIEWS, alpha outside 0..256,
 * n_palette < 1 (4 with a target) or > 65536, a view rectangle larger than the canvas, t_max negative or NaN, an
 * unknown flag.
 * ------------------------------------------------------------------------ */
typedef struct OccdMapRenderArgs {
    const uint8_t* labels;         /* (n_rows, 4096) device                                                   */
    const uint8_t* target;         /* (n_rows, 4096), or NULL: class mode                                     */
    const int32_t* cells;          /* (gx, gy, gz) row of the brick, negative = absent                        */
    const OccdRenderView* views;   /* (n_views) device, window voxel units                                    */
    const uint8_t* palette;        /* (n_palette, 3) device                                                   */
    const uint8_t* background;     /* (n_views, H, W, 3), or NULL                                             */
    uint8_t* rgb;                  /* (n_views, H, W, 3)                                                      */
    int64_t* hit;                  /* (n_views, H, W) row * 4096 + local voxel or -1, or NULL                 */
    uint8_t* face;                 /* (n_views, H, W) as OccdRenderArgs.face, or NULL                         */
    float* depth;                  /* (n_views, H, W) t at the hit, +inf on a miss, or NULL                   */
    int32_t gx, gy, gz, n_rows;
    int32_t n_views, H, W;
    int32_t n_palette, alpha;
    int32_t flags;
    float t_max;                   /* +inf: no limit                                                          */
    int32_t view_w[OCCD_RENDER_MAX_VIEWS], view_h[OCCD_RENDER_MAX_VIEWS];
    uint8_t bg_colour[4];
} OccdMapRenderArgs;
int occd_map_render(const OccdMapRenderArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K34: which voxels of a frame the camera could see (occd_frame_visibility, csrc/visibility.hip).  Additive
 * (OCCD_ABI_VERSION note).  One ray per pixel of ONE view through ONE frame's label volume, one thread per pixel, a wave
 * per 8 x 8 pixel tile.  `view` is one OccdRenderView in grid-voxel units, read exactly as occd_render_voxels reads it,
 * and the walk is that of occd_render_voxels in class mode (csrc/raycast.h holds it, expression for expression: same
 * ray set-up, slab entry, clamped first voxel, boundary
 * times ((float)(i + (dir > 0)) - origin) * (1 / dir), x before y before z on ties, step bound X + Y + Z + 3, float32
 * without fma).  Every voxel n the walk visits, up to and including the first occupied one (0 < label < 255), gets
 * visible[n] = 1; a ray that leaves the grid has marked all it crossed; a ray that misses the box marks nothing.  Every
 * other byte of visible is 0: the entry point zeroes the volume itself with a fill kernel on the same stream (no memset
 * node).  All writers of a byte write the same value (plain byte stores, a byte that already reads 1 is not written
 * again), so the result depends on the inputs alone.  No read-modify-write atomics, no allocation, no host sync
 * (capture-safe).  Visibility is pixel-centric on purpose: a voxel is visible when some pixel's ray reaches it, not when
 * the ray to its centre is free (that rule hides nearly all distant ground behind the ground in front of it).
 * hit, when not NULL: hit[v W + u] = the first occupied voxel (x Y + y) Z + z of pixel (u, v), or -1 -- what
 * occd_render_voxels writes to its hit for the same view.
 * OCCD_EINVAL before any launch: a NULL argument, NULL labels / view / visible, non-positive H, W, X, Y or Z,
 * X Y Z > 2^28, label_bytes not 1 or 2.
 * ------------------------------------------------------------------------ */
typedef struct OccdVisibilityArgs {
    const void* labels;            /* (X Y Z) labels of the frame, label_bytes each                           */
    const OccdRenderView* view;    /* one view, device, grid-voxel units                                      */
    uint8_t* visible;              /* (X Y Z) out: 1 = a pixel ray reached the voxel, else 0                  */
    int32_t* hit;                  /* (H, W) out: first occupied voxel or -1, or NULL                         */
    int32_t H, W;
    int32_t X, Y, Z;
    int32_t label_bytes;
} OccdVisibilityArgs;
int occd_frame_visibility(const OccdVisibilityArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * Weighted votes for the sequence map (csrc/semantic_map.hip).  Additive (OCCD_ABI_VERSION note): the unweighted
 * entry points and their structs are unchanged, and both kinds of vote may go into one pool -- saturating sums of
 * non-negative weights commute, so extraction, merge, save / load and render apply as they are.
 *
 * occd_map_integrate_weighted is occd_map_integrate with a REQUIRED (X Y Z) uint8 `weight` volume where that one has its
 * optional mask: the frame voxel n votes with w = weight[n], the counter becomes min(v + w, 65535), and w == 0 casts no
 * vote.  Every other rule (geometry, label < C, slots, table_host) is occd_map_integrate's.  With weights in {0, 1} the
 * pool bytes equal those of occd_map_integrate with that volume as the mask.
 *
 * occd_map_sample_weighted is occd_map_sample with `own_weight` where that one has own_mask.  OCCD_MAP_SAMPLE_EXCLUDE_SELF
 * retracts w = own_weight[n'] from the counter own[n'] iff n' is inside (X, Y, Z), own[n'] < C, w > 0, and the counter v
 * has v != 65535 and v >= w (a saturated counter has forgotten what it dropped; a counter below w cannot hold that
 * vote); for w = 1 this is occd_map_sample's rule.  own_weight is read only under that flag and is then required.
 * n_obs and min_obs are sums of counters, so with weighted votes they are in VOTE UNITS (a frame that voted with
 * weight 8 adds 8), not in frames.
 * OCCD_EINVAL before any launch: what the unweighted entry refuses, a NULL weight (integrate), EXCLUDE_SELF without
 * own_weight (sample).
 * ------------------------------------------------------------------------ */
typedef struct OccdMapWeightedArgs {
    uint16_t* votes;               /* (capacity, 4096, pitch) vote counters                                          */
    const int32_t* table;          /* (n_bricks, 16) device                                                          */
    const int32_t* table_host;     /* the same rows in host memory, or NULL                                          */
    const void* labels;            /* (X Y Z) labels of the frame, label_bytes each                                  */
    const uint8_t* weight;         /* (X Y Z) bytes, the weight of each voxel's vote, 0 = does not vote              */
    int32_t n_bricks, capacity;
    int32_t X, Y, Z;
    int32_t C, pitch, label_bytes;
} OccdMapWeightedArgs;
int occd_map_integrate_weighted(const OccdMapWeightedArgs* a, void* stream);

typedef struct OccdMapSampleWeightedArgs {
    const uint16_t* votes;         /* (capacity, 4096, pitch) vote counters, read only                               */
    const int32_t* table;          /* (n_bricks, 16) device                                                          */
    const int32_t* table_host;     /* the same rows in host memory, or NULL                                          */
    const int32_t* cells;          /* (gx, gy, gz) device: row of the brick, negative = absent                       */
    const void* own;               /* (X Y Z) labels of the frame itself, label_bytes each, or NULL                  */
    const uint8_t* own_weight;     /* (X Y Z) bytes, the weights the frame voted with; NULL without EXCLUDE_SELF     */
    uint8_t* labels;               /* (X Y Z) out                                                                    */
    uint16_t* n_obs;               /* (X Y Z) out, vote units                                                        */
    int32_t n_bricks, capacity;
    int32_t X, Y, Z;
    int32_t gx, gy, gz;
    int32_t C, pitch, label_bytes;
    int32_t min_obs, flags;        /* min_obs in vote units                                                          */
    int32_t Bq[9], dq[3];          /* row-major rint(R 2^16), rint(d 2^16)                                           */
} OccdMapSampleWeightedArgs;
int occd_map_sample_weighted(const OccdMapSampleWeightedArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K35: score a prediction along sensor rays (occd_ray_metric, csrc/ray_metric.hip): the counters of RayIoU ("Fully
 * Sparse 3D Occupancy Prediction", Liu et al., 2024).  Additive (OCCD_ABI_VERSION note).  One thread per (frame b,
 * origin k, ray r), 64 consecutive rays a wave: ray r of origin k of frame b is origins[b, k] + t dirs[r], in grid-voxel
 * units (voxel (i, j, l) is the cube [i, i + 1) x [j, j + 1) x [l, l + 1)), through pred[b] and target[b], both
 * (X, Y, Z) with z fastest.
 * The walk is that of occd_render_voxels in class mode (csrc/raycast.h: slab entry, clamped first voxel, boundary times
 * ((float)(i + (dir > 0)) - origin) * (1 / dir), x before y before z on ties, step bound X + Y + Z + 3, float32
 * without fma), ONE walk for both volumes: every visited voxel is tested in whichever volume has not hit yet, and the
 * walk ends when both have hit or the ray leaves the grid -- the voxel sequence depends on the ray alone, so the outcome
 * is that of two independent casts.  A hit is the first voxel with 0 < label < 255; its depth is the t at which the ray
 * entered that voxel (0 when the origin lies in it): what occd_render_voxels writes to `depth`.  A non-finite origin
 * or direction component makes the ray a miss in both volumes.
 * Target label 255 (unknown): with unknown_mode OCCD_RAY_UNKNOWN_DROP a ray that meets a target voxel 255 before its
 * target hit is counted in `unknown` and nowhere else but `rays`; with OCCD_RAY_UNKNOWN_PASS 255 is transparent, as it
 * always is in the prediction.  (2-byte labels above 255 are transparent in both volumes and both modes.)
 * counts: int64, ADDED to (never zeroed; the caller zeroes it outside a capture or with a fill kernel).  With C =
 * n_classes and T = n_thresholds, OCCD_RAY_COUNTERS + 2 C + T C + T entries:
 *   [0] rays       every ray cast, B K N per call
 *   [1] valid      the target hit a class 1 .. C - 1 (and the ray was not dropped); only these rays are scored
 *   [2] unknown    rays dropped under OCCD_RAY_UNKNOWN_DROP
 *   [3] pred_miss  valid rays on which the prediction hit nothing
 *   [4 + c]                  gt[c]      valid rays whose target hit has class c
 *   [4 + C + c]              pred[c]    valid rays whose prediction hit has class c < C
 *   [4 + 2 C + k C + c]      tp[k][c]   valid rays, both hits of class c, fabsf(t_pred - t_target) < thresholds[k]
 *   [4 + 2 C + T C + k]      tp_geo[k]  valid rays, any prediction hit, fabsf(t_pred - t_target) < thresholds[k]
 * A hit label >= C (other than 255) reaches no per-class counter: such a target hit leaves the ray out of `valid`, such a
 * prediction hit on a valid ray is no pred_miss, may count in tp_geo, and counts in no pred[c].  Counters are u32 in LDS
 * per workgroup, then one integer atomic per non-zero counter: the sums do not depend on the schedule.  No allocation,
 * no host sync, no memset node (capture-safe).
 * OCCD_EINVAL before any launch: a NULL argument, NULL pred / target / origins / dirs / counts, non-positive batch,
 * n_origins, n_rays, X, Y or Z, pred_bytes or target_bytes not 1 or 2, n_thresholds outside 1 .. 4, n_classes outside
 * 1 .. 32, an unknown_mode other than the two above, X Y Z >= 2^31, batch n_origins n_rays >= 2^31.
 * ------------------------------------------------------------------------ */
#define OCCD_RAY_MAX_THRESHOLDS 4
#define OCCD_RAY_MAX_CLASSES 32
#define OCCD_RAY_UNKNOWN_DROP 0
#define OCCD_RAY_UNKNOWN_PASS 1
#define OCCD_RAY_COUNTERS 4 /* rays, valid, unknown, pred_miss: the scalar counters in front of the per-class ones */
typedef struct OccdRayMetricArgs {
    const void* pred;              /* (B, X, Y, Z) predicted labels, pred_bytes each                          */
    const void* target;            /* (B, X, Y, Z) target labels, target_bytes each                           */
    const float* origins;          /* (B, K, 3) ray origins, grid-voxel units                                 */
    const float* dirs;             /* (N, 3) ray directions, shared by every origin and frame                 */
    int64_t* counts;               /* (OCCD_RAY_COUNTERS + 2 C + T C + T) counters, added to                  */
    int32_t batch, n_origins, n_rays;
    int32_t X, Y, Z;
    int32_t pred_bytes, target_bytes;
    int32_t n_classes, n_thresholds, unknown_mode;
    float thresholds[OCCD_RAY_MAX_THRESHOLDS];   /* grid-voxel units: metres / voxel size                    */
} OccdRayMetricArgs;
int occd_ray_metric(const OccdRayMetricArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K36: the depth-rendering loss (csrc/render_loss.hip).  Additive (OCCD_ABI_VERSION note).  The soft occupancy of the
 * logits is alpha-composited along one camera's pixel rays into an expected depth image d^, which is held to a metric
 * depth map D; forward and backward in four kernels that share one argument struct (every kernel reads the fields it
 * names below and ignores the rest).
 *
 * Volume: logits z, element (b, c, s) at b*s_b + c*s_c + s*s_v floats, the layouts of occd_ssc_loss_stats_*_strided
 * ((s_c, s_v) = (S, 1) planes, or (1, cs) channels-last rows with cs % 4 == 0, s_b % 4 == 0 and a 16-byte aligned base,
 * read with 16-byte loads); S = X Y Z, voxel s = (x*Y + y)*Z + z; class 0 is empty; 2 <= C <= 32.
 * Opacity: a_v = 1 - softmax(z_v)[0], formed as min(1, sum_{c > 0} p_c) so that it does not cancel when p_0 -> 1.  The
 * opacity buffer holds it in a SIGNED form that keeps the relative precision of both a and 1 - a in 4 bytes: s = a where
 * a <= 1/2, s = -p_0 where a > 1/2 (-0.0f where p_0 < 2^-25: a rounds to 1, the voxel is opaque); the ray passes read
 * a = s or 1 + s and 1 - a = 1 - s or -s by the sign BIT.  (1 - a formed from a float32 a near 1 carries ulp(1) / (1 - a) of
 * relative error into every transmittance behind the voxel and into the voxel's own gradient: 6e-6 at a = 0.99.)  A
 * buffer of plain non-negative opacities is read as what it says.
 * Rays: ray (i, j) of frame b is pixel (u, v) = (off_u + stride*i, off_v + stride*j) of the (H, W) image of view b
 * (OccdRenderView, 18 floats): origin and direction are formed from (float)u + 0.5f, (float)v + 0.5f exactly as
 * occd_render_voxels forms them, so a strided pass walks rows off_v::stride and columns off_u::stride of the full
 * pass's rays bit for bit.  h = ceil((H - off_v) / stride), w = ceil((W - off_u) / stride), h*w <= 2^21.  t along a ray
 * is whatever the view makes it (camera depth in metres for render.camera_view).
 * Walk: that of occd_render_voxels (csrc/raycast.h: slab entry, clamped first voxel, boundary times
 * ((float)(i + (dir > 0)) - origin) * (1 / dir), x before y before z on ties, step bound X + Y + Z + 3, float32 without
 * fma).  It visits voxels v_1 .. v_n
 * with entry depths t_1 <= .. <= t_n (t_1 = the slab entry, 0 when the origin lies inside) and ends when the ray leaves
 * the grid or the next entry depth is >= max_depth (no voxel at all when t_1 >= max_depth).  t_end = min(t_far,
 * max_depth), t_far the slab exit; max_depth for a ray that misses the grid (it renders empty).
 * Compositing, float32: T_1 = 1, w_i = T_i a_i, T_{i+1} = T_i (1 - a_i), d^ = sum_i w_i t_i + T_{n+1} t_end (summed in
 * walk order); the rendered opacity is 1 - T_{n+1}.  The depth of a voxel is its ENTRY t: with hard logits d^ is the
 * depth occd_render_voxels reports, bit for bit.  No path-length weighting.  The walk may stop once T is exactly 0:
 * everything behind is weighted by an exact zero.
 * Target: gt_depth element (b, v, u) at b*d_b + v*d_h + u*d_w floats (read in place at the ray's pixel, no resampled
 * copy), 0 = no measurement.  A ray is valid when it passes the slab test, D is finite, 0 < D <= max_depth and D > t_1.
 * D_r = min(D, t_end).  l_r = omega_r |d^_r - D_r|, omega_r = 1 (OCCD_RENDER_LOSS_ABS) or 1 / max(D_r, 0.25)
 * (OCCD_RENDER_LOSS_REL; the floor bounds the fixed-point sums below).
 *   stats[0] = sum over valid rays of l_r (Q24: (u64)(l_r 2^24 + 0.5) each), stats[1] = #valid rays; zeroed by the
 *   forward with a kernel; L = stats[0] / 2^24 / max(1, stats[1]).  LDS first, one integer atomic per workgroup.
 * Backward, without a division: with pre_k = sum_{i <= k} w_i t_i,  d d^ / d a_k * (1 - a_k) = T_{k+1} t_k - (d^ - pre_k),
 * and every d a_v / d z_{v,c} carries the factor p_0 = 1 - a_v.  The ray pass re-walks each valid ray in forward order
 * with the saved d^ and adds  omega_r sign(d^_r - D_r) [T_{k+1} t_k - (d^_r - pre_k)]  (sign(0) = 0; float32, then
 * rint(x 2^32)) into hsum (B, S) int64 with one 8-byte integer atomic per visited voxel, zero contributions skipped:
 * |term| <= 4 * 128 = 2^9 over at most 2^21 rays, |H| < 2^62.  The voxel pass writes
 *   grad(b, c, s) = gscale[0] * H_v 2^-32 * p_c  (c > 0),   -gscale[0] * H_v 2^-32 * a_v  (c = 0)
 * to element b*g_b + c*g_c + s*g_v (channels-last rows: channels [C, g_pad) written as zeros, as
 * occd_ssc_loss_stats_bwd_strided) and stores 0 back into hsum: zero it once at allocation and it is clean after every
 * backward, in captured replays too.  gscale: device scalar g / max(1, #valid).  Integer sums: loss and gradient do not
 * depend on the schedule.  No allocation, no host sync, no memset node (capture-safe).
 *   occd_render_opacity           reads logits (+ strides, C);                         writes opacity (B, S), signed form
 *   occd_render_depth_fwd         reads opacity, views, gt_depth (NULL: render only, stats NULL too);
 *                                 writes depth (B, h, w), alpha (B, h, w), stats[2]
 *   occd_render_depth_bwd_rays    reads opacity, views, gt_depth, depth;                adds into hsum
 *   occd_render_depth_bwd_voxels  reads logits, hsum, gscale;                           writes grad, zeroes hsum
 * OCCD_EINVAL before any launch: a NULL argument or a NULL pointer the kernel reads or writes, batch outside 1 .. 256,
 * non-positive X, Y or Z, X Y Z >= 2^31, C outside 2 .. 32, strides the strided ssc kernels would refuse, non-positive H,
 * W or stride, an offset outside [0, stride) or outside the image, h or w that are not the two quotients above,
 * h*w > 2^21, max_depth not in (0, 128], a norm other than the two above, negative depth-map strides, gt_depth without
 * stats or stats without gt_depth, a g_pad the ssc backward would refuse.
 * ------------------------------------------------------------------------ */
#define OCCD_RENDER_LOSS_ABS 0
#define OCCD_RENDER_LOSS_REL 1
typedef struct OccdRenderLossArgs {
    const float* logits;           /* (B, C, S) through (s_b, s_c, s_v)                                       */
    float* opacity;                /* (B, S), the signed form                                                 */
    const float* views;            /* (B, 18): one OccdRenderView per frame                                   */
    const float* gt_depth;         /* (B, H, W) through (d_b, d_h, d_w), or NULL                              */
    float* depth;                  /* (B, h, w) d^: written by the forward, read by the backward ray pass     */
    float* alpha;                  /* (B, h, w) rendered opacity 1 - T_{n+1}                                  */
    int64_t* stats;                /* [sum of l_r (Q24), #valid rays]                                         */
    int64_t* hsum;                 /* (B, S) H, Q32                                                           */
    const float* gscale;           /* device scalar g / max(1, #valid)                                        */
    float* grad;                   /* d L / d logits through (g_b, g_c, g_v)                                  */
    int64_t s_b, s_c, s_v;
    int64_t g_b, g_c, g_v;
    int64_t d_b, d_h, d_w;
    int32_t batch, C, X, Y, Z;
    int32_t H, W, h, w;
    int32_t stride, off_u, off_v;
    int32_t g_pad, norm;
    float max_depth;
} OccdRenderLossArgs;
int occd_render_opacity(const OccdRenderLossArgs* a, void* stream);
int occd_render_depth_fwd(const OccdRenderLossArgs* a, void* stream);
int occd_render_depth_bwd_rays(const OccdRenderLossArgs* a, void* stream);
int occd_render_depth_bwd_voxels(const OccdRenderLossArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K37: exact truncated squared Euclidean distance transform of label volumes (occd_edt_sq) and the counters of the
 * distance-tolerant scores -- precision, recall and F-score at a distance, Chamfer distance -- made of it
 * (occd_dist_metric); csrc/edt.hip.  Additive (OCCD_ABI_VERSION note).
 *
 * Definitions.  A label volume is (B, X, Y, Z), z fastest, 1 or 2 bytes per label (uint8, or the uint16 values
 * occd_argmax_channels writes).  Classes are 0 .. C - 1 with 0 free, C = n_classes <= OCCD_EDT_MAX_CLASSES.
 *   Slot s of a volume is a seed set: slot 0 = every voxel with 1 <= label < C (occupied), slot c >= 1 = every voxel
 *   with label == c.  A label >= C (255 included) is never a seed.
 *   D_s(v) = min(min over the seeds u of slot s of |v - u|^2, T + 1): integer, in voxel units, T = max_d2 the caller's
 *   truncation, 1 <= T <= 65534.  A volume without a seed of the slot has T + 1 everywhere.  Frames are independent.
 * Truncation is exact under the separable passes (z, then y, then x, each out[i] = min(min_k in[i + k] + k^2, T + 1)): a
 * candidate more than floor(sqrt(T)) away along an axis cannot give a value <= T and a saturating add stays saturated, so
 * no pass looks further than that window.  Integer arithmetic only: nothing depends on the schedule.
 *
 * occd_edt_sq: labels -> dist (B, n_slots, X, Y, Z) uint16, dist[b][i] = D_{slots[i]} of labels[b].  scratch: at least
 *   2 B n_slots X Y Z bytes (one plane set beside `dist`).  target, mask, counts, target_bytes are ignored.
 * occd_dist_metric: labels = the prediction, target, optional byte mask (B, X, Y, Z) -> counts, int64
 *   [2][C][T + 2], ADDED to (never zeroed; the caller zeroes it outside a capture).  A voxel v is a QUERY iff
 *   target(v) != 255 and, with a mask, mask(v) != 0.
 *     side 0: for every query v and every slot s whose PREDICTION seed set contains v: counts[0][s][D_s^target(v)] += 1
 *     side 1: for every query v and every slot s whose TARGET seed set contains v:     counts[1][s][D_s^pred(v)] += 1
 *   Seeds are not masked: only queries are restricted.  Bin T + 1 is "further than T, or no seed at all".
 *   The x pass feeds the counters directly (u32 LDS histograms of T + 2 bins where T + 2 <= 4096, one 64-bit integer
 *   atomic per non-zero bin; above that one atomic per counted voxel); D is never written.  The 2 C (side, slot)
 *   pairs of a frame are processed OCCD_EDT_CHUNK at a time.  scratch: at least 4 OCCD_EDT_CHUNK X Y Z bytes (two sets
 *   of OCCD_EDT_CHUNK uint16 planes of one frame), whatever B and C.  dist, slots, n_slots are ignored.
 * No allocation, no host sync, no memset node (capture-safe).
 * OCCD_EINVAL before any launch: a NULL argument, NULL labels / scratch, NULL dist (edt_sq), NULL target / counts
 * (dist_metric), non-positive batch, X, Y or Z, label_bytes (target_bytes) not 1 or 2, n_classes outside 1 .. 32, max_d2
 * outside 1 .. 65534, X^2 + Y^2 + Z^2 >= 2^31, B X Y Z >= 2^31, scratch_bytes below the sizes above, n_slots outside
 * 1 .. 32, a slot outside 0 .. C - 1, B n_slots > 65535, B n_slots X Y Z >= 2^40.
 * ------------------------------------------------------------------------ */
#define OCCD_EDT_MAX_CLASSES 32
#define OCCD_EDT_CHUNK 8 /* (side, slot) pairs of a frame occd_dist_metric transforms per group of launches */
typedef struct OccdEdtArgs {
    const void* labels;            /* (B, X, Y, Z) labels, label_bytes each; dist_metric: the prediction      */
    const void* target;            /* (B, X, Y, Z) target labels, target_bytes each (dist_metric)             */
    const uint8_t* mask;           /* (B, X, Y, Z) query mask or NULL (dist_metric)                           */
    uint16_t* dist;                /* (B, n_slots, X, Y, Z) squared distances (edt_sq)                        */
    int64_t* counts;               /* [2][C][T + 2] counters, added to (dist_metric)                          */
    void* scratch;                 /* intermediate planes                                                     */
    int64_t scratch_bytes;
    int32_t batch, X, Y, Z;
    int32_t label_bytes, target_bytes;
    int32_t n_classes, max_d2, n_slots;
    int32_t slots[OCCD_EDT_MAX_CLASSES];
} OccdEdtArgs;
int occd_edt_sq(const OccdEdtArgs* a, void* stream);
int occd_dist_metric(const OccdEdtArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K38: stable segmented key/value radix sort (csrc/sort.hip).  Additive (OCCD_ABI_VERSION note).
 * Sorts `segments` independent rows of n (uint32 key, uint32 value) pairs each, ascending on key bits
 * [begin_bit, end_bit) (the other bits are carried along and do not take part); pairs whose keys agree on those bits keep
 * their input order (stable), so the result is numpy.argsort(kind="stable") of the masked keys, exactly.
 * LSD radix sort, OCCD_SORT_RADIX_BITS bits a pass (the last pass takes what is left), passes =
 * ceil((end_bit - begin_bit) / OCCD_SORT_RADIX_BITS), ping-pong between buffer 0 (keys, vals: the input, overwritten)
 * and buffer 1 (keys_alt, vals_alt): THE RESULT IS IN BUFFER passes % 2.  Each pass is three launches: digit histograms
 * of every tile of OCCD_SORT_TILE pairs, one exclusive scan per segment over the (digit, tile) table, and a scatter that
 * ranks a tile's pairs (wave-wide match on the digit's bits with ballots, per-wave digit counters in LDS, the tile
 * reordered through LDS so that a digit's run leaves as one stretch).  No kernel waits for another workgroup; the launch
 * geometry depends on (segments, n) only; no allocation, no host read, no memset node: capture-safe, and the output does
 * not depend on the schedule (no floating point, every position is a sum of counts).
 * hist: workspace of segments * 2^OCCD_SORT_RADIX_BITS * ceil(n / OCCD_SORT_TILE) uint32.
 * OCCD_EINVAL before any launch: a NULL argument or pointer, n outside 1 .. 2^31 - 1, segments outside 1 .. 65535,
 * segments * n >= 2^40, a bit range that is not 0 <= begin_bit < end_bit <= 32.
 * ------------------------------------------------------------------------ */
#define OCCD_SORT_TILE 4096
#define OCCD_SORT_RADIX_BITS 8
typedef struct OccdSortArgs {
    uint32_t* keys;                /* (segments, n) buffer 0: the input                                       */
    uint32_t* vals;
    uint32_t* keys_alt;            /* (segments, n) buffer 1                                                  */
    uint32_t* vals_alt;
    uint32_t* hist;                /* workspace, see above                                                    */
    int64_t n;
    int32_t segments, begin_bit, end_bit;
} OccdSortArgs;
int occd_sort_pairs_u32(const OccdSortArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * The Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018) on top of K38 (csrc/lovasz.hip).  Additive.  Over the whole
 * batch (per_image = False) and the classes present in the target.  N = batch * S voxels, voxel i = b * S + s; logits
 * element (b, c, s) at b*s_b + c*s_c + s*s_v floats, the two layouts of occd_ssc_loss_stats_*_strided; target (N,) uint8,
 * the label `ignore` is unknown.  For class c and valid voxel i: fg = [y_i == c], p = softmax(z_i)[c] in float32 (expf),
 * e = fg ? sum_{c' != c} p_c' : p, clamped to [0, 1] (1 - p formed without cancellation: a saturated voxel gives an exact
 * 0).  G_c = #fg.  The valid voxels of class c are ordered by DESCENDING e, ties by ASCENDING voxel index.  For the element
 * at sorted position k, with F = #fg strictly before it and b = #bg up to and including it, the Jaccard increment is
 *   g = 1 / (G + b)  (fg),      g = (G - F) / ((G + b - 1)(G + b))  (bg),      g = 0 for every element when G = 0,
 * evaluated in float64 from the integer counters with IEEE division and rounded once to float32.
 *   L_c = sum_k e_(k) g_k,  L = (1 / #present) sum_{G_c > 0} L_c,  d L / d p_{i,c} = (fg ? -1 : +1) g / #present.
 * L_c is accumulated as integers in Q60: every term is rint(e * g64 * 2^60), g64 the float64 g before its rounding to
 * float32, added with 64-bit integer atomics (LDS, then one per workgroup), so loss_q does not depend on the schedule.  Terms lie in [0, 1] and sum to at most 1 (the Jaccard index),
 * so the sum stays below 2^61.  WORST-CASE ROUNDING of L_c against exact arithmetic on the same float32 errors:
 *   N * 2^-61 (half a unit per term)  +  2^-50 (the float64 roundings of g, e g and the scaling, relative, on terms that
 *   sum to at most 1).
 *   occd_lovasz_errors  reads logits, target; for classes c0 .. c0 + cc - 1 writes segment c - c0 of keys, vals (cc, N):
 *                       key = 0x3F800000 - bits(e) (ascending key = descending e; 30 bits), OCCD_LOVASZ_INVALID_KEY for
 *                       an unknown voxel (behind every valid one; sort bits [0, OCCD_LOVASZ_KEY_BITS)); val = i | fg << 31
 *   occd_lovasz_ranks   reads the SORTED keys, vals; three launches (fg sums per tile of OCCD_LOVASZ_RANK_TILE, one scan
 *                       per segment, apply); writes fg_count[c0 + j] = G, loss_q[c0 + j] (zeroed by a kernel first),
 *                       q[i * C + c0 + j] = (fg ? -g : g) for every valid voxel (voxel-major); tsum: workspace of
 *                       cc * ceil(N / OCCD_LOVASZ_RANK_TILE) uint32
 *   occd_lovasz_bwd     reads logits, target, q (N, C), gscale (device scalar: incoming gradient / #present); writes
 *                       grad(b, j, s) = gscale p_j (q_j - sum_c q_c p_c) through (g_b, g_c, g_v), zeros for an unknown
 *                       voxel (q is not read there) and for the pad channels [C, g_pad) of channels-last rows
 * OCCD_EINVAL before any launch: a NULL argument or a pointer the kernel uses, batch or S non-positive, N >= 2^31, C outside
 * 2 .. 32, c0 / cc outside the classes, strides or a g_pad the strided ssc kernels would refuse.
 * ------------------------------------------------------------------------ */
#define OCCD_LOVASZ_Q 60
#define OCCD_LOVASZ_KEY_BITS 31
#define OCCD_LOVASZ_INVALID_KEY 0x40000000
#define OCCD_LOVASZ_RANK_TILE 2048
typedef struct OccdLovaszArgs {
    const float* logits;           /* (B, C, S) through (s_b, s_c, s_v)                                       */
    const uint8_t* target;         /* (B, S)                                                                  */
    uint32_t* keys;                /* (cc, N)                                                                 */
    uint32_t* vals;                /* (cc, N)                                                                 */
    uint32_t* tsum;                /* workspace of the ranks pass                                             */
    float* q;                      /* (N, C) signed Jaccard increments                                        */
    int64_t* fg_count;             /* (C) G_c                                                                 */
    int64_t* loss_q;               /* (C) L_c, Q60                                                            */
    const float* gscale;           /* device scalar                                                           */
    float* grad;                   /* d L / d logits through (g_b, g_c, g_v)                                  */
    int64_t s_b, s_c, s_v;
    int64_t g_b, g_c, g_v;
    int64_t S;
    int32_t batch, C, c0, cc;
    int32_t g_pad, ignore;
} OccdLovaszArgs;
int occd_lovasz_errors(const OccdLovaszArgs* a, void* stream);
int occd_lovasz_ranks(const OccdLovaszArgs* a, void* stream);
int occd_lovasz_bwd(const OccdLovaszArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K39: the surface of a brick volume as an indexed quad mesh (csrc/mesh.hip).  Additive (OCCD_ABI_VERSION note).
 * Input: the volume occd_map_render draws -- labels (n_rows, 4096) uint8, one row per 16^3 brick, voxel (i, j, l) of a
 * brick at (i*16 + j)*16 + l, and the directory cells (gx, gy, gz) int32, the row of the brick at that cell or negative.
 * Only rows the directory points to are meshed; a row named by several cells is meshed at the lowest of them.
 * Solid: label in 1..254.  Free: label 0.  Unknown: label 255, a voxel of an absent brick (cells < 0 or >= n_rows) and a
 * voxel outside the window.  A solid voxel emits the face towards direction d when the neighbour there is free, or when
 * it is unknown and cap_unknown != 0; a neighbour that is solid (of any class) gives no face.
 * Face code d = 2 * axis + side: axis 0 / 1 / 2 = x / y / z is the code of occd_render_voxels' `face` buffer (d >> 1),
 * side 0 is the face at the voxel's lower coordinate (outward normal -e_axis), side 1 the one at its upper (+e_axis):
 *   0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z.
 * Output, in window lattice units (corner (x, y, z), 0 <= x <= 16 gx ...; voxel (x, y, z) spans [x, x + 1] ...):
 *   faces, F of them, ascending in (row, brick-local voxel index, face code): face_label (F) the voxel's label, face_dir (F)
 *   the code, quads (F, 4) the vertex indices of the corners, counter-clockwise seen from outside, starting at the
 *   lexicographically smallest corner c0: with b = (axis + 1) % 3, c = (axis + 2) % 3 the corners are c0, c0 + e_b,
 *   c0 + e_b + e_c, c0 + e_c on side 1 and c0, c0 + e_c, c0 + e_c + e_b, c0 + e_b on side 0, so that
 *   (v1 - v0) x (v3 - v0) is the outward normal;
 *   vertices (V, 3) int32: every lattice corner some face uses, once, ascending in (x, y, z).
 * Every array is a function of the input alone (every position is a sum of counts; the one atomic, a minimum, has an
 * order-free result).  Corner key = x << (by + bz) | y << bz | z, b* = bit_length(16 g*); key_bits = bx + by + bz.
 * The stages (the caller scans between them and sorts with occd_sort_pairs_u32):
 *   occd_mesh_count  writes row_cell (n_rows; workspace: the cell of each row or a value outside the directory, read
 *                    again by occd_mesh_emit) and counts[row] = the faces of that row.  One workgroup per row stages the
 *                    brick and the facing planes of its six neighbours in LDS.
 *   occd_mesh_emit   reads row_cell and offsets (the exclusive scan of counts); writes face_label, face_dir and, for
 *                    corner k of face f, keys_lo[4 f + k] = the key's low 32 bits, keys_hi[4 f + k] = its high bits
 *                    (only when key_bits > 32), refs[4 f + k] = 4 f + k.  No entry at or past n_faces is written.
 *   occd_mesh_heads  reads keys_lo (keys_hi) SORTED by key; marks[p] = 1 where p = 0 or key[p] != key[p - 1], else 0.
 *   occd_mesh_weld   reads the sorted keys_lo (keys_hi), refs and ranks (the inclusive scan of marks): quads[refs[p]] =
 *                    ranks[p] - 1, and where ranks[p] differs from ranks[p - 1] (or p = 0) vertices[ranks[p] - 1] = the
 *                    unpacked key.  A ref >= 4 n_faces or a rank outside 1 .. n_vertices writes nothing.
 * No allocation, no host sync, no memset node (capture-safe).
 * OCCD_EINVAL before any launch: a NULL argument or a pointer the stage uses (keys_hi only when key_bits > 32), labels,
 * keys_lo or refs not 16-byte aligned, gx, gy or gz outside 1 .. OCCD_MESH_MAX_GRID, gx gy gz > OCCD_MESH_MAX_CELLS,
 * n_rows <= 0, key_bits > OCCD_MESH_MAX_KEY_BITS, an entry of cells_host (the directory's host copy, optional) >= n_rows;
 * emit, heads, weld: n_faces <= 0 or 4 n_faces >= 2^31 (the n of occd_sort_pairs_u32); weld: n_vertices <= 0.
 * ------------------------------------------------------------------------ */
#define OCCD_MESH_MAX_GRID 65536       /* bricks along one axis: the limits of occd_map_render's directory */
#define OCCD_MESH_MAX_CELLS 134217728  /* 2^27 */
#define OCCD_MESH_MAX_KEY_BITS 63
typedef struct OccdMeshArgs {
    const uint8_t* labels;         /* (n_rows, 4096) device                                                   */
    const int32_t* cells;          /* (gx, gy, gz) device: row of the brick, negative = absent                */
    const int32_t* cells_host;     /* optional host copy of cells, checked before the launch                  */
    int32_t* row_cell;             /* (n_rows) workspace: count writes, emit reads                            */
    int32_t* counts;               /* count: (n_rows)                                                         */
    const int64_t* offsets;        /* emit: (n_rows) exclusive prefix sum of counts                           */
    uint8_t* face_label;           /* emit: (F)                                                               */
    uint8_t* face_dir;             /* emit: (F)                                                               */
    uint32_t* keys_lo;             /* (4 F) emit writes; heads, weld read them sorted                         */
    uint32_t* keys_hi;             /* (4 F) likewise, key_bits > 32 only                                      */
    uint32_t* refs;                /* (4 F) emit writes 4 f + k; weld reads them sorted                       */
    int32_t* marks;                /* heads: (4 F)                                                            */
    const int32_t* ranks;          /* weld: (4 F) inclusive prefix sum of marks                               */
    int32_t* quads;                /* weld: (F, 4)                                                            */
    int32_t* vertices;             /* weld: (V, 3)                                                            */
    int64_t n_faces;               /* F = the sum of counts                                                   */
    int64_t n_vertices;            /* V = ranks[4 F - 1]                                                      */
    int32_t gx, gy, gz, n_rows;
    int32_t cap_unknown;
} OccdMeshArgs;
int occd_mesh_count(const OccdMeshArgs* a, void* stream);
int occd_mesh_emit(const OccdMeshArgs* a, void* stream);
int occd_mesh_heads(const OccdMeshArgs* a, void* stream);
int occd_mesh_weld(const OccdMeshArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * K40: connected components of a label volume (csrc/ccl.hip).  Additive (OCCD_ABI_VERSION note).
 * Input: labels (B, X, Y, Z) uint8, z fastest, N = X Y Z < 2^31 - 1 voxels a frame; the B frames are independent.  Two
 * class masks of 256 bits (bit l of a mask = word l >> 5, bit l & 31), disjoint, either may be empty:
 *   things: a segment is a maximal set of voxels of one and the same class that is connected under `connectivity`
 *           (6: faces; 26: faces, edges and corners).  With `instances` (B, X, Y, Z) int32 given, a segment is instead
 *           every voxel of the frame with one and the same instance id in 1 .. N - 1 (ids <= 0 or >= N belong to no
 *           segment); an id that carries more than one class sets OCCD_CCL_STATUS_INSTANCE.
 *   stuff:  a segment is every voxel of that class in the frame, as one.
 * A label in neither mask (0 and 255 too, unless a mask names them) belongs to no segment.
 * seg (B, X, Y, Z) int32: 0 where the voxel belongs to no segment, else 1 + the smallest linear index, within the frame,
 * of any voxel of its segment.  This canonical form makes seg a function of the input alone, whatever the schedule.
 *
 * occd_ccl_segments: labels -> seg, four launches.  (1) fill: stuff_min = INT32_MAX, *status = 0.  (2) tile-local: one
 *   workgroup per OCCD_CCL_TILE^3 tile stages the tile's labels in LDS and unites every pair of neighbouring things voxels
 *   of one class inside the tile (union-find in LDS: a root is the smallest index of its tree, links go from the larger
 *   root to the smaller with an LDS atomic minimum), then writes parent[v] = the frame-linear index of the root of v (-1
 *   for a voxel outside things) and lowers stuff_min[b][class] with one atomic minimum per class present in the tile.
 *   (3) seam: one thread per voxel unites it with each of its "earlier" neighbours (3 of 6, 13 of 26) of the same class
 *   that lies in ANOTHER tile.  parent only ever decreases and every value ever stored in parent[v] is a voxel of v's
 *   true component, so a stale read can only name an older ancestor: find() reads with agent-scope atomic loads, and a
 *   link is made only by atomicMin(parent + hi, lo), which took effect as a link iff it returns hi (hi was a root at that
 *   instant); otherwise the union goes on from the value returned.  A stale read costs a retry, never a wrong merge.
 *   (4) flatten, a launch of its own (it reads parent only after the launch boundary): seg = 1 + root, or 1 +
 *   stuff_min[b][class], or 0.  With OCCD_CCL_NO_TILE_PASS in flags (2) is replaced by parent[v] = v and (3) unites
 *   every pair: the same seg, for measurements.  No kernel waits for another workgroup.  Every loop that depends on the
 *   data is bounded: a find by N + 1 steps (4097 in LDS), a union by N + 1 retries (parents strictly decrease); a
 *   kernel that overruns sets OCCD_CCL_STATUS_OVERRUN in *status and goes on to its end without spinning; the caller
 *   reads *status when it next synchronises.
 *   Workspace: parent B N int32, stuff_min 256 B int32, status 1 int32.
 * occd_ccl_roots: seg -> marks (B, N) int32, 1 at the voxel whose index + 1 is its seg (one per segment), else 0.
 * occd_ccl_compact: seg, ranks (B, N) int32 = the inclusive scan of marks within each frame, offsets (B) int64 = the
 *   exclusive scan over the frames of count[b] = ranks[b][N - 1], n_segments = the sum of count -> ids (B, N) int32, the
 *   segments of a frame numbered 1 .. count[b] in ascending order of seg, 0 kept; and, for segment k of frame b at row
 *   offsets[b] + k - 1 of the tables (n_segments rows): seg_class its class, seg_index its smallest voxel index, seg_size
 *   its voxels (integer atomic adds on zeroed rows: the order does not matter).  n_segments = 0: ids only.
 * occd_ccl_filter: labels, seg -> out (B, X, Y, Z) uint8, a copy of labels in which every voxel of a things segment of
 *   fewer than min_voxels voxels is 0; stuff and every other voxel pass.  Workspace: parent, B N int32 (the sizes).
 * Integer arithmetic only; no allocation, no host read, no memset node (capture-safe).
 * OCCD_EINVAL before any launch: a NULL argument or a pointer the stage uses, batch, X, Y or Z < 1, batch > 65535, N >=
 * 2^31 - 1, B N >= 2^40, connectivity not 6 or 26 (segments), masks that overlap, min_voxels < 1 (filter), n_segments < 0.
 * ------------------------------------------------------------------------ */
#define OCCD_CCL_TILE 16
#define OCCD_CCL_NO_TILE_PASS 1        /* flags: seam pass over every voxel pair */
#define OCCD_CCL_STATUS_OVERRUN 1      /* *status: a bounded loop ran out (a bug or a corrupted workspace) */
#define OCCD_CCL_STATUS_INSTANCE 2     /* *status: an instance id carries more than one class */
typedef struct OccdCclArgs {
    const uint8_t* labels;         /* (B, X, Y, Z)                                                            */
    const int32_t* instances;      /* (B, X, Y, Z) or NULL (segments)                                         */
    int32_t* parent;               /* workspace (B, N): segments, filter                                      */
    int32_t* stuff_min;            /* workspace (B, 256): segments                                            */
    int32_t* status;               /* device word: segments                                                   */
    int32_t* seg;                  /* (B, N): segments writes; roots, compact, filter read                    */
    int32_t* marks;                /* roots: (B, N)                                                           */
    const int32_t* ranks;          /* compact: (B, N)                                                         */
    const int64_t* offsets;        /* compact: (B)                                                            */
    int32_t* ids;                  /* compact: (B, N)                                                         */
    uint8_t* seg_class;            /* compact: (n_segments)                                                   */
    int32_t* seg_size;             /* compact: (n_segments)                                                   */
    int32_t* seg_index;            /* compact: (n_segments)                                                   */
    uint8_t* out;                  /* filter: (B, X, Y, Z)                                                    */
    int64_t n_segments;
    int32_t batch, X, Y, Z;
    int32_t connectivity, min_voxels, flags;
    uint32_t things[8], stuff[8];
} OccdCclArgs;
int occd_ccl_segments(const OccdCclArgs* a, void* stream);
int occd_ccl_roots(const OccdCclArgs* a, void* stream);
int occd_ccl_compact(const OccdCclArgs* a, void* stream);
int occd_ccl_filter(const OccdCclArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * The overlaps of two segment-id volumes, counted exactly (csrc/ccl.hip, on K38).  Additive.  g_ids, p_ids (B, N) int32:
 * the `ids` of occd_ccl_compact for the target and the prediction of the same frames; g_offsets, p_offsets (B) int64 its
 * `offsets`.  A voxel is valid iff target != 255 and, with a mask, mask != 0.  The GLOBAL id of a segment is offsets[b] +
 * id (1-based over the batch), 0 = no segment.  For every ordered pair (g, p) of global ids, not both 0, that some valid
 * voxel carries: one row (g, p, n), n = the number of such voxels; rows ascending in (g, p).  M = B N < 2^31.
 *   occd_ccl_pair_marks  marks[i] = 1 where voxel i is valid and lies in a segment of either volume, else 0.
 *   occd_ccl_pair_emit   pos = the inclusive scan of marks over all M voxels, n_pairs = pos[M - 1]: for a marked voxel
 *                        at q = pos[i] - 1: keys_lo[q] = g << p_bits | p when keys_hi is NULL (g_bits + p_bits <= 32),
 *                        else keys_lo[q] = p, keys_hi[q] = g; refs[q] = q.
 *   (the caller sorts by key with occd_sort_pairs_u32: one stage over p_bits + g_bits, or p_bits then g_bits)
 *   occd_ccl_pair_heads  the SORTED keys -> marks[q] = 1 where q = 0 or key[q] != key[q - 1].
 *   occd_ccl_pair_rows   the sorted keys and ranks = the inclusive scan of those marks, n_rows = ranks[n_pairs - 1] ->
 *                        row_g, row_p, row_n (n_rows); row_start (n_rows) is workspace.  Two launches.
 * No allocation, no host read, no memset node.  OCCD_EINVAL before any launch: a NULL argument or a pointer the stage uses,
 * batch or n < 1, batch n >= 2^31, p_bits outside 1 .. 32 or > 31 without keys_hi, n_pairs or n_rows < 1 where the stage
 * reads them.
 * ------------------------------------------------------------------------ */
typedef struct OccdCclPairArgs {
    const int32_t* g_ids;          /* (B, N) marks, emit                                                      */
    const int32_t* p_ids;          /* (B, N)                                                                  */
    const uint8_t* target;         /* (B, N) labels: 255 = not valid                                          */
    const uint8_t* mask;           /* (B, N) or NULL                                                          */
    const int64_t* g_offsets;      /* (B) emit                                                                */
    const int64_t* p_offsets;      /* (B) emit                                                                */
    int32_t* marks;                /* marks: (B N); heads: (n_pairs)                                          */
    const int32_t* pos;            /* emit: (B N)                                                             */
    uint32_t* keys_lo;             /* (n_pairs) emit writes; heads, rows read them sorted                     */
    uint32_t* keys_hi;             /* (n_pairs) or NULL                                                       */
    uint32_t* refs;                /* (n_pairs) emit                                                          */
    const int32_t* ranks;          /* rows: (n_pairs)                                                         */
    int32_t* row_start;            /* rows: workspace (n_rows)                                                */
    int32_t* row_g;                /* rows: (n_rows)                                                          */
    int32_t* row_p;
    int32_t* row_n;
    int64_t n;                     /* N, voxels a frame                                                       */
    int64_t n_pairs, n_rows;
    int32_t batch, p_bits;
} OccdCclPairArgs;
int occd_ccl_pair_marks(const OccdCclPairArgs* a, void* stream);
int occd_ccl_pair_emit(const OccdCclPairArgs* a, void* stream);
int occd_ccl_pair_heads(const OccdCclPairArgs* a, void* stream);
int occd_ccl_pair_rows(const OccdCclPairArgs* a, void* stream);

/* ------------------------------------------------------------------------ *
 * In-library kernel timing (HIP events on the launch stream) used by bench.py
 * for `roofline.achieved`.  occd_prof_enable(1) starts recording one event pair
 * per launch; occd_prof_report() synchronises the recorded events and returns,
 * per kernel tag, launches / total ms / total algorithmic flops / bytes.
 * ------------------------------------------------------------------------ */
typedef struct occd_prof_row {
    char tag[64];
    int64_t launches;
    double ms;
    double flops;
    double bytes;
} occd_prof_row;

int occd_prof_enable(int32_t on);
int occd_prof_set_tag(const char* tag);   /* tag attached to subsequent launches */
int occd_prof_report(occd_prof_row* rows, int32_t max_rows); /* returns #rows; resets */

#ifdef __cplusplus
}
#endif
#endif /* OCCDEPTH_AMD_H */
