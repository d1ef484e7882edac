/*
 * cofi_hip.h — C ABI of libcofi_hip.so: the MI355X (gfx950) kernels behind CoFiI2P's
 * coarse-to-fine correspondence forward path.
 *
 * The reference (WHU-USI3DV/CoFiI2P) is pure Python/PyTorch and has NO FFI/plugin layer
 * (SURVEY.md §8b); the drop-in boundary is its nn.Module surface (model/network.py:14-164).
 * This header is the kernel-level boundary underneath that surface: each entry point replaces
 * one stock-op sequence of the reference, cited as `file:line` (paths relative to the reference
 * root).  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / torch CUDA tensor .data_ptr()) unless the
 *     parameter name ends in `_host`;
 *   - all matrices are row-major fp32 with an explicit leading dimension `ld*` in ELEMENTS;
 *   - neighbour/index tables are int32 on the device (`cofi_idx64_to_idx32` converts the
 *     reference's int64 tables once per frame);
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on it, allocates
 *     nothing, keeps no global state and is re-entrant;
 *   - scratch memory is passed in (`ws`, `ws_bytes`), sized by the matching `*_workspace` query;
 *   - STACK MODE: entry points with a `frames` parameter process `frames` equally sized frames stacked along the
 *     row axis in one launch; N / M / L / S / H / W are then PER-FRAME sizes, index tables hold frame-local
 *     indices, per-frame statistics / scales are laid out (frames, ...).  frames = 1 is the single-frame case.
 *     Row-wise entry points (GEMM, LayerNorm, L2 norm, position embedding, fused layer tail) need no such
 *     parameter: call them with the stacked row count;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     COFI_E* code for argument errors (nothing is launched in that case).
 */
#ifndef COFI_HIP_H
#define COFI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cofi_split_bf16_planes (nplanes), cofi_transpose (frames) and cofi_select_matches (frames) gained positional arguments (round 4);
 * a caller built against version 1 must not bind this library */
#define COFI_ABI_VERSION 3

#define COFI_EINVAL (-1)      /* bad shape / alignment / null pointer */
#define COFI_EWORKSPACE (-2)  /* workspace too small */
#define COFI_EUNSUPPORTED (-3)

typedef void *cofi_stream_t;

/* A PENDING normalisation: an activation y (rows, channels) whose GroupNorm / InstanceNorm (+ affine + LeakyReLU) has not been
 * applied yet, described by the statistics partials its producer left behind.  Producers (cofi_gemm_f32_colstats / _fused,
 * cofi_conv2d_nhwc / _fused) write, per 64-row slab and per `width` adjacent output columns, {sum, sum of squares}:
 *   partials (nslab, channels / width, 2) fp32, nslab = frames * ceil(rows_per_frame / 64)  (other slab heights: `slab_rows`).
 * Consumers (cofi_gemm_f32_fused, cofi_conv2d_nhwc_fused, cofi_group_norm_apply_partials) fold the table themselves
 * (fixed order, fp64) and evaluate   leaky( (y - mean_g) * rstd_g * gamma[c] + beta[c], slope ),  g = c / (channels / groups),
 * i.e. nn.GroupNorm(groups, channels) over ALL rows of the frame (model/kpconv/modules.py:45-48) or, with groups == channels and
 * gamma == NULL, the affine-less InstanceNorm of model/imagenet.py:123 / model/network.py:42-43.
 * width, channels / width and groups are powers of two; width divides channels / groups. */
typedef struct cofi_norm_desc {
    const float *partials;
    int nslab;    /* all frames */
    int width;    /* output columns per table entry */
    int channels;
    int groups;
    const float *gamma, *beta; /* (channels) or both NULL */
    float eps;
    float slope;  /* LeakyReLU slope in [0, 1]: 1 = identity, 0 = ReLU, 0.1 = the reference's LeakyReLU */
    const float *scale_shift; /* optional (frames, 2, channels): the statistics already FINALIZED by cofi_norm_finalize into per-channel
                               * scale[c] = rstd_g gamma[c] | shift[c] = beta[c] - mean_g rstd_g gamma[c]; consumers then skip their own fold */
    int slab_rows; /* rows per slab of the producer: 0 = 64 (GEMM / convolution epilogues); cofi_kpconv_fused writes 64-, 32- or 16-row slabs
                    * (cofi_kpconv_fused_slab_rows).  nslab = frames * ceil(rows_per_frame / slab_rows); consumers only sum over the slabs */
} cofi_norm_desc_t;

/* activation codes of the GEMM epilogue */
#define COFI_ACT_NONE 0
#define COFI_ACT_RELU 1
#define COFI_ACT_SIGMOID 2
#define COFI_ACT_LEAKY01 3 /* LeakyReLU(0.1), the point encoder's activation (model/kpconv/modules.py:85,142,222) */
/* OR-ed into `act` (or into `relu` of cofi_gemm_f32_layernorm): form the fp32 products as a 3-term bf16 split
 * (hi*hi + hi*lo + lo*hi, fp32 accumulate) on the bf16 matrix cores instead of the exact fp32 MFMA:
 * ~2^-16 relative error per product, 5.3x the MFMA rate. */
#define COFI_GEMM_BF16X3 0x100
/* with COFI_GEMM_BF16X3 / COFI_GEMM_BF16X6: W is PRE-SPLIT (cofi_split_bf16_planes with 2 / 3 planes): `W` points at the bf16 hi plane, N rows
 * of `ldw` bf16 (ldw % 8 == 0, rows zero-padded past K), immediately followed by the lo plane (bf16x6: the mid plane, then the lo plane) of
 * the same shape.  Weights are static: splitting them once removes half of the on-the-fly conversion work of every launch. */
#define COFI_GEMM_W_SPLIT 0x200
/* with COFI_GEMM_W_SPLIT, cofi_gemm_f32_fused only: A is PRE-SPLIT too - `A` points at its bf16 hi plane, M rows of `lda` bf16
 * (lda % 8 == 0, K % 8 == 0), immediately followed by the lo plane (M * lda elements later): what cofi_kpconv_aggregate writes with
 * planes = 1.  Both operands then travel global -> LDS by LDS-DMA (global_load_lds) through a software-pipelined multi-stage ring
 * (csrc/gemm_planes.inc: 9 tile configurations, plans tuned on MI355X); same products, same K order as the other bf16x3 kernels - equal
 * split-K gives equal bits.  Not combinable with a_norm. */
#define COFI_GEMM_A_SPLIT 0x400
/* fp32-GRADE arithmetic on the bf16 matrix cores: every fp32 operand is split on the fly into THREE bf16 planes (hi + mid + lo = all 24
 * mantissa bits) and the product formed as hi*hi + hi*mid + mid*hi + mid*mid + hi*lo + lo*hi with fp32 accumulation - what is dropped is
 * below 2^-24 of |a||b|, so the result differs from an exact-fp32 contraction only by accumulation-order rounding (measured: same error
 * against fp64 as the fp32 MFMA kernel) at 16/6 = 2.7x its matrix rate.  A is split on the fly (no COFI_GEMM_A_SPLIT); W is fp32 or - with
 * COFI_GEMM_W_SPLIT - three pre-split planes; the normalising loader (a_norm) works with both.  Accepted by cofi_gemm_f32*, cofi_conv2d_nhwc*. */
#define COFI_GEMM_BF16X6 0x800
/* OR-ed into `act` of cofi_gemm_f32_fused / cofi_conv2d_nhwc_fused (N <= 128): every output row is L2-normalised after bias, residual
 * and activation - y = v / max(|v|, 1e-12), F.normalize(dim=1) of model/network.py:83-84, 90 - in the epilogue (a tile, or the split-K
 * reduction, spans the whole row): the stand-alone cofi_l2norm_rows pass over the output disappears. */
#define COFI_GEMM_L2NORM 0x1000
/* with COFI_GEMM_BF16X6: the LARGE contractions (the shapes that take the 256 x 128 one-workgroup-per-CU kernel: N >= 128, M >= 256,
 * K % 32 == 0, fp32 W, no fused LayerNorm / L2 norm) may run in the three-product fp16 split instead of the six-product bf16 split:
 * operand = fp16 hi + fp16 lo of x * 2^e (22-24 significant bits), products lo*hi + hi*lo + hi*hi on the fp16 matrix instruction, fp32
 * accumulation - fp32-grade like COFI_GEMM_BF16X6 (same or smaller error against fp64) at half the matrix work.  The power-of-two
 * scales are kept per workgroup panel INSIDE the kernel (chosen from the first K-tile, verified on every tile, the tile re-split and the
 * accumulators rescaled - exactly - when a tile leaves the fp16 window): no caller-side range information, no extra pass, deterministic
 * bits.  csrc/gemm_f16_big.inc.  Shapes that do not take that kernel ignore the flag (bf16x6 as before). */
#define COFI_GEMM_F16X3 0x2000
/* with COFI_GEMM_F16X3, for launches that take its kernel (ask cofi_gemm_f16x3_eligible / cofi_conv2d_f16x3_eligible first; any other launch
 * returns COFI_EUNSUPPORTED): W is a STATIC operand split once - an (N, ldw) buffer of the fp32 matrix's shape in which every aligned group of
 * four values w[n][4 g .. 4 g + 3] is replaced by eight fp16 {hi0 hi1 hi2 hi3 lo0 lo1 lo2 lo3}, hi = f16(w s), lo = f16(w s - hi), s = the power
 * of two of the row's 128-row panel that puts the panel's largest |w| into [2^11, 2^12) (1 for an all-zero panel); the ceil(N / 128) panel
 * scales follow the matrix as fp32 at W[N * ldw ...].  The kernel then copies W's planes instead of splitting them in each of its M / 256
 * workgroups (cofii2p_amd.ops.pack_f16x3_weight builds the buffer). */
#define COFI_GEMM_W_F16PRE 0x4000

int cofi_abi_version(void);
/* name of the code object's target, "gfx950" */
const char *cofi_target_arch(void);

/* ---------------------------------------------------------------------------------------------
 * K1  brute-force KNN with wavefront top-k.
 * Replaces model/kpconv/preprocess_data.py:109-143 (`square_distance` + `knn`, i.e.
 * dist.topk(k, largest=False)) and model/network.py:250-264 (`point2node`, k = 1).
 * support (S,3), query (Q,3) fp32 contiguous.  out_idx (Q,k) int32, ascending by
 * (distance, index): ties are broken by the LOWEST support index (torch.topk leaves them
 * unspecified).  Distance arithmetic is the canonical fp32 sequence documented in
 * oracle/knn_oracle.c.  If S < k the tail of a row is padded with the shadow index S.
 * out_dist (Q,k) may be NULL.  k <= 128.
 */
int cofi_knn_topk(const float *support, int S, const float *query, int Q, int k, int32_t *out_idx, float *out_dist,
                  cofi_stream_t stream);
/* The same search (identical out_idx / out_dist, bit for bit) over a uniform 2-D cell grid of the support set: a query
 * visits only the cells that can hold one of its k nearest (cofii2p_amd/csrc/knn_grid.hip states the pruning bound).
 *   cofi_knn_grid_workspace(S)   bytes of `ws` (16-byte aligned device memory)
 *   cofi_knn_grid_build(...)     bounding box, <= 128 x 128 cells of about 12 points, counting sort into cell order; optional
 *                                order_out (S) int32 = the support indices in cell order (a spatially coherent query order
 *                                for a self search)
 *   cofi_knn_topk_grid(...)      wave per query against a built grid; qorder (Q) optional: wave w handles query qorder[w]
 * One grid serves every search against that support set (neighbors[i], subsampling[i], upsampling[i-1] of
 * preprocess_data.py:60-99 share stage i).  Worth it from a few thousand support points on; below that cofi_knn_topk. */
/* Column 0 of upsampling[i] (the nearest stage-(i+1) point of every stage-i point; the only column the forward reads, functional.py:20)
 * WITHOUT a search: stage i+1 is a selection with replacement of stage i (sub[j] = stage-i index of point j, S1 entries), so the answer
 * is the first selected entry of the point's own sorted row neighbors[i] (N, k) - ties at the minimal canonical distance resolved to the
 * lowest stage-(i+1) index, exactly as cofi_knn_topk* would.  first_copy: N int32 of scratch.  out_idx[p * ldo] = that index. */
int cofi_knn_up_nearest(const float *points, int N, const int32_t *neighbors, int k, const int32_t *sub, int S1, int32_t *first_copy,
                        int32_t *out_idx, int ldo, cofi_stream_t stream);
size_t cofi_knn_grid_workspace(int S);
int cofi_knn_grid_build(const float *support, int S, void *ws, size_t ws_bytes, int32_t *order_out, cofi_stream_t stream);
int cofi_knn_topk_grid(const void *ws, size_t ws_bytes, int S, const float *query, const int32_t *qorder, int Q, int k,
                       int32_t *out_idx, float *out_dist, cofi_stream_t stream);
int cofi_nearest_node(const float *nodes, int S, const float *points, int Q, int32_t *out_idx, cofi_stream_t stream);
/* like cofi_nearest_node, but the query rows are points_all[sel[i]] for i < *count_dev (count read
 * on the device: no host sync).  Used by the test-mode matching chain (network.py:152-153). */
int cofi_nearest_node_sel(const float *nodes, int S, const float *points_all, const int32_t *sel, const int32_t *count_dev,
                          int max_count, int32_t *out_idx, cofi_stream_t stream);

/* int64 -> int32 index tables (values must fit; the shadow index N is preserved) */
int cofi_idx64_to_idx32(const int64_t *src, int32_t *dst, size_t n, cofi_stream_t stream);
int cofi_idx32_to_idx64(const int32_t *src, int64_t *dst, size_t n, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2  KPConv, part 1: kernel-point influence + neighbour aggregation (MFMA 16x16x4 f32).
 * Replaces model/kpconv/kpconv.py:91-105:
 *   w[m,h,k] = max(0, 1 - |(s_pts[idx[m,h]] - q_pts[m]) - kp[k]| / sigma)
 *   agg[m, k*C + c] = sum_h w[m,h,k] * feats[idx[m,h], c]
 * and kpconv.py:113-115: cnt[m] = max(1, #{h : row_pos[idx[m,h]] != 0}) (as float), where
 * row_pos[n] = (sum_c feats[n,c] > 0) comes from cofi_row_sum_positive.
 * idx (M,H) int32; idx == N is the shadow neighbour (far point, zero feature).  H % 4 == 0.
 * agg is (M, 15*C) with leading dimension ld_agg; part 2 is cofi_gemm_f32 with `rowdiv = cnt`.
 */
int cofi_row_sum_positive(const float *feats, int ld, int N, int C, uint8_t *row_pos, cofi_stream_t stream);
/* First layer (C <= 4 feature channels, e.g. [intensity | normal]): the cost of a neighbour in the staging is the number of cache lines
 * its data lies in, so features, position and the positive-sum flag of every support point are packed ONCE into 32-byte records
 * (N, 8) = [f0 f1 f2 f3 | x y z | flag] (cofi_kp_pack_c4, replaces cofi_row_sum_positive for this layer) and cofi_kpconv_aggregate_c4
 * gathers one record per neighbour.  Same operands and order as cofi_kpconv_aggregate: identical results. */
int cofi_kp_pack_c4(const float *feats, int ldf, int C, const float *points /* (N,3) */, int N, float *records, cofi_stream_t stream);
int cofi_kpconv_aggregate_c4(const float *records, int N, int C, const float *q_pts, const int32_t *idx, int M, int H,
                             const float *kernel_points, float sigma, float *agg, int ld_agg, float *cnt, int frames,
                             const int32_t *order, cofi_stream_t stream);
int cofi_kpconv_aggregate(const float *feats, int ldf, int N, int C, const float *q_pts, const float *s_pts, const int32_t *idx,
                          int M, int H, const float *kernel_points /* (15,3) */, float sigma, const uint8_t *row_pos,
                          float *agg, int ld_agg, int agg_planes /* 0: fp32 (M, ld_agg); 1: bf16 hi plane (M, ld_agg bf16, ld_agg % 8 == 0,
                          C % 4 == 0) followed by the lo plane - the operand form of COFI_GEMM_A_SPLIT */,
                          float *cnt, int frames, const int32_t *order /* optional (frames*M) frame-local
                          processing order of the queries, e.g. Morton-sorted: results do not depend on it */,
                          cofi_stream_t stream);
/* The support as ONE 16-byte record per row, (frames * N, 4) floats = (x, y, z, flag), 16-byte aligned, flag = 1.0f where row_pos
 * would be 1: the staging then costs one gather per neighbour instead of four.  The records come from the GroupNorm apply that
 * produced feats (cofi_group_norm_apply_rec / _partials_rec) or, for any other feats, from cofi_kp_pack_support (N = all rows; the
 * flag is cofi_row_sum_positive's).  cofi_kpconv_aggregate_rec = cofi_kpconv_aggregate with `records` in place of s_pts and row_pos:
 * the same kernels, the same results. */
int cofi_kp_pack_support(const float *feats, int ldf, int N, int C, const float *points /* (N,3) */, float *records, cofi_stream_t stream);
int cofi_kpconv_aggregate_rec(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records, const int32_t *idx,
                              int M, int H, const float *kernel_points, float sigma, float *agg, int ld_agg, int agg_planes, float *cnt,
                              int frames, const int32_t *order, cofi_stream_t stream);
/* SORTED index tables.  Where the caller promises that in every row of idx the entries inside [0, N) come first, in ascending order of
 * the canonical fp32 distance of the KNN kernels (cofi_knn: ((-2 q.s) + |q|^2) + |s|^2), and entries outside [0, N) only behind them,
 * the neighbours inside the kernel's support are a prefix of the row: the _sorted entry points gather the records of that prefix only
 * (neighbours 0 - 15, then 16 - 63, then 64 - 127, as far as something behind can still be inside) and take the positive-sum flags of
 * all H neighbours from a bit table, (frames, cofi_kp_bits_words(N)) 32-bit words written by cofi_kp_pack_bits from the records
 * (stride = floats per record: 4 for support records, 8 for the first layer's; the flag is the record's last float).  Same results as
 * the unsorted entry points, bit for bit, on every table that keeps the promise; on any other table the result is undefined. */
int cofi_kp_bits_words(int N);
int cofi_kp_pack_bits(const float *records, int stride, int N, int frames, uint32_t *bits, cofi_stream_t stream);
int cofi_kpconv_aggregate_rec_sorted(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records, const uint32_t *bits,
                                     const int32_t *idx, int M, int H, const float *kernel_points, float sigma, float *agg, int ld_agg,
                                     int agg_planes, float *cnt, int frames, const int32_t *order, cofi_stream_t stream);
int cofi_kpconv_aggregate_c4_sorted(const float *records, const uint32_t *bits, int N, int C, const float *q_pts, const int32_t *idx, int M, int H,
                                    const float *kernel_points, float sigma, float *agg, int ld_agg, float *cnt, int frames,
                                    const int32_t *order, cofi_stream_t stream);

/* KPConv as ONE kernel for the narrow layers (C = 32 or 64 = in = out channels, the stages with the most queries):
 *   y[m] = (sum_k agg[m, k, :] W[k]) / max(#neighbours whose feature row sums to > 0, 1) + bias       (kpconv.py:91-116)
 * with agg as cofi_kpconv_aggregate computes it - but the (M, 15 C) aggregate (39 MB per layer at these stages) stays in LDS as bf16
 * hi / lo planes and is multiplied there with the pre-split weight planes (3-term bf16 split on the bf16 matrix cores, fp32
 * accumulation; w_planes = hi plane (C rows x ldw bf16, K index = kernel point * C + channel, i.e. the (Cout, 15 Cin) packing the
 * GEMM path uses) followed by the lo plane, cofi_split_bf16_planes).  colpart != NULL: GroupNorm statistics partials of y per
 * slab of cofi_kpconv_fused_slab_rows(C, M, frames) rows and `stat_width` adjacent columns.  M % 16 == 0, H % 4 == 0;
 * COFI_EUNSUPPORTED for other shapes (use cofi_kpconv_aggregate + cofi_gemm_f32_fused). */
int cofi_kpconv_fused_slab_rows(int C, int M, int frames);
int cofi_kpconv_fused(const float *feats, int ldf, int N, int C, const float *q_pts, const float *s_pts, const int32_t *idx, int M, int H,
                      const float *kernel_points, float sigma, const uint8_t *row_pos, const void *w_planes, int ldw, const float *bias,
                      float *y, int ldy, float *colpart, int stat_width, int frames, const int32_t *order, cofi_stream_t stream);
/* cofi_kpconv_fused with the support as 16-byte records (see cofi_kpconv_aggregate_rec) in place of s_pts and row_pos */
int cofi_kpconv_fused_rec(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records, const int32_t *idx, int M, int H,
                          const float *kernel_points, float sigma, const void *w_planes, int ldw, const float *bias, float *y, int ldy,
                          float *colpart, int stat_width, int frames, const int32_t *order, cofi_stream_t stream);
/* cofi_kpconv_fused_rec for sorted index tables (see cofi_kpconv_aggregate_rec_sorted) */
int cofi_kpconv_fused_rec_sorted(const float *feats, int ldf, int N, int C, const float *q_pts, const float *records, const uint32_t *bits,
                                 const int32_t *idx, int M, int H, const float *kernel_points, float sigma, const void *w_planes, int ldw,
                                 const float *bias, float *y, int ldy, float *colpart, int stat_width, int frames, const int32_t *order,
                                 cofi_stream_t stream);
/* K3 / K4  neighbour max-pool and nearest up-sample.
 * Replace model/kpconv/functional.py:53-66 (`maxpool`) and :5-21 (`nearest_upsample`): a zero
 * pad row stands behind index N. */
int cofi_neighbor_maxpool(const float *x, int ldx, int N, int C, const int32_t *idx, int M, int H, float *out, int ldo, int frames,
                          const int32_t *order /* optional, as above */, cofi_stream_t stream);
/* cofi_neighbor_maxpool for a source that fits a CU's LDS a few channels at a time (the deep stages of a stack-mode submission): one
 * workgroup per (frame, group of 8 or 4 channels, range of queries) loads the frame's N x 8 (N + 2 <= 3072, C > 4) or N x 4
 * (N + 2 <= 6144) slice once, coalesced, and serves all H neighbours of its queries from LDS.  Same bits as cofi_neighbor_maxpool (a
 * maximum is exact in any order) - on every table without the entry INT_MIN: that kernel keeps INT_MIN as its own mark for "past the end
 * of the row" and ignores such an entry, here it is an index outside [0, N) like any other and lists the zero row.  Any C, ldx, ldo and alignment (16-byte loads and stores where they are aligned); `order` is accepted
 * and ignored.  COFI_EUNSUPPORTED where the slice does not fit at 4 channels - cofi_neighbor_maxpool_slice_ok(N, C, H, frames) says
 * (1 / 0) whether a launch would be served. */
int cofi_neighbor_maxpool_slice_ok(int N, int C, int H, int frames);
int cofi_neighbor_maxpool_slice(const float *x, int ldx, int N, int C, const int32_t *idx, int M, int H, float *out, int ldo, int frames,
                                const int32_t *order /* ignored */, cofi_stream_t stream);
int cofi_gather_rows(const float *x, int ldx, int N, int C, const int32_t *idx, int idx_stride, int M, float *out, int ldo, int frames,
                     cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dense contraction on fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 products/accumulation.
 *   C[m,n] = act( (sum_k A[m,k] * W[n,k]) / rowdiv[m] + bias[n] )
 * A (M,K) lda; W (N,K) ldw — torch.nn.Linear's own layout, so weights are used in place
 * (model/kpconv/modules.py:76 `nn.Linear`, model/transformer/transformer.py:27-37,
 * model/network.py:29,42-43; KPConv weights (15,Cin,Cout) are packed once to (Cout, 15*Cin),
 * kpconv.py:107-110).  K % 4 == 0, lda % 4 == 0, ldw % 4 == 0, 16-byte aligned bases.
 * bias / rowdiv may be NULL.  Deep-K problems are split over K into `ws` and reduced in a fixed
 * order (deterministic, no float atomics) by a fold launch.  Launches that run CONCURRENTLY (different streams) need different workspaces.
 */
/* 1 if a COFI_GEMM_BF16X6 | COFI_GEMM_F16X3 launch of this shape (fp32 operands, no fused LayerNorm / L2 norm; pending_norm: A carries a
 * pending normalisation, `frames` stacked frames) runs on the f16x3 kernel - i.e. may be given a COFI_GEMM_W_F16PRE weight. */
int cofi_gemm_f16x3_eligible(int M, int N, int K, int pending_norm, int frames);
int cofi_conv2d_f16x3_eligible(int H, int W, int Cin, int Cout, int ks, int stride, int pad, int ldx, int pending_norm, int frames);
size_t cofi_gemm_f32_workspace(int M, int N, int K);
int cofi_gemm_f32(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K, const float *bias,
                  const float *rowdiv, int act, void *ws, size_t ws_bytes, cofi_stream_t stream);
/* Split a static fp32 operand W (N,K) ldw once into bf16 planes for COFI_GEMM_W_SPLIT: planes = (nplanes, N, ldp) bf16,
 * nplanes = 2 (COFI_GEMM_BF16X3): [hi = bf16(W) RNE | lo = bf16(W - hi)]; nplanes = 3 (COFI_GEMM_BF16X6): [hi | mid = bf16(W - hi) |
 * lo = bf16(W - hi - mid)] - the roundings of the kernels' own on-the-fly split, so a pre-split launch is bit-identical to one that
 * splits W itself.  ldp % 8 == 0, ldp >= K, rows zero-padded; 16-byte aligned. */
int cofi_split_bf16_planes(const float *W, int ldw, int N, int K, void *planes, int ldp, int nplanes, cofi_stream_t stream);
/* Same contraction with fused COLUMN STATISTICS: colpart (nslab, N, 2) receives, per row slab, the sum and
 * the sum of squares of every output column (after bias / rowdiv / act), nslab =
 * cofi_gemm_f32_stat_slabs(M,N,K).  cofi_group_stats_from_colpart / cofi_col_inv_norm_from_colpart turn
 * them into GroupNorm statistics (modules.py:45-48) or the token-axis Q scale (transformer.py:53) without
 * re-reading the activation. */
int cofi_gemm_f32_stat_slabs(int M, int N, int K);
int cofi_gemm_f32_colstats(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K,
                           const float *bias, const float *rowdiv, int act, float *colpart, void *ws, size_t ws_bytes,
                           cofi_stream_t stream);
/* The general form.  a_norm != NULL: A is the RAW output of the previous layer and its pending normalisation (see
 * cofi_norm_desc_t; channels == K) is applied by the operand loader - the normalised activation never exists in memory
 * (replaces the GroupNorm + LeakyReLU between two Linear layers, modules.py:45-49,89-94,232-236).  Needs COFI_GEMM_BF16X3 |
 * COFI_GEMM_W_SPLIT, K <= 512; in stack mode M / frames must be a multiple of 128.  COFI_EUNSUPPORTED otherwise (apply the
 * normalisation with cofi_group_norm_apply_partials first).
 * colpart != NULL: statistics partials of C with one entry per `stat_width` adjacent columns, (nslab, N / stat_width, 2);
 * stat_width a power of two <= 64 dividing N (the GroupNorm group width C/32 keeps the table at 256 bytes per slab). */
int cofi_gemm_f32_fused(const float *A, int lda, const cofi_norm_desc_t *a_norm, const float *W, int ldw, float *C, int ldc, int M, int N,
                        int K, const float *bias, const float *rowdiv, int act, float *colpart, int stat_width, void *ws, size_t ws_bytes,
                        int frames, cofi_stream_t stream);
/* cofi_gemm_f32_fused with a RESIDUAL joined in the epilogue, before the activation, the statistics and the L2 normalisation:
 *   C[m,:] = act( (A W^T)[m,:] / rowdiv[m] + bias + R[m,:] ),   R[m,:] = res[m,:]                                  (res_idx == NULL)
 *                                                                R[m,:] = res[f * res_rows + res_idx[m * res_idx_stride], :]  otherwise,
 * f = m / (M / frames) the frame of row m: the indices are frame-local and an index outside [0, res_rows) is a shadow point whose
 * residual is zero - the conventions of cofi_gather_rows, so Linear(cat[x[idx], y]) = (x W_up^T)[idx] + y W_skip^T + b runs as two
 * contractions and the gathered matrix never exists (the FPN decoders, model/kpconv/kp_backbone.py:111-124).  res (rows of ldr >= N
 * floats) holds frames * res_rows rows when indexed, M rows otherwise.  Everything cofi_gemm_f32_fused accepts is accepted; the residual
 * is added once, by the fold launch, when K is split.  res == NULL: cofi_gemm_f32_fused, bit for bit.
 * COFI_EINVAL: res_idx without res, ldr < N, and with an index table res_rows <= 0, res_idx_stride <= 0, M % frames != 0 or
 * frames * res_rows > INT_MAX (source rows are addressed with an int). */
int cofi_gemm_f32_fused_res(const float *A, int lda, const cofi_norm_desc_t *a_norm, const float *W, int ldw, float *C, int ldc, int M, int N,
                            int K, const float *bias, const float *rowdiv, int act, float *colpart, int stat_width, void *ws, size_t ws_bytes,
                            int frames, const float *res, int ldr, const int32_t *res_idx, int res_idx_stride, int res_rows,
                            cofi_stream_t stream);
/* Contraction with fused row LayerNorm (N <= 128): C = relu?(LN(A W^T + bias) * gamma + beta) + res.
 * Replaces Linear + nn.LayerNorm (+ residual) of model/transformer/transformer.py:57-58,61-64. */
int cofi_gemm_f32_layernorm(const float *A, int lda, const float *W, int ldw, float *C, int ldc, int M, int N, int K,
                            const float *bias, const float *gamma, const float *beta, float eps, int relu, const float *res, int ldr,
                            void *ws, size_t ws_bytes /* cofi_gemm_f32_workspace(M,N,K) */, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K5  stack-mode GroupNorm (+ LeakyReLU / residual).
 * Replaces model/kpconv/modules.py:32-49 (nn.GroupNorm over ALL rows of the frame x C/groups
 * channels, eps 1e-5, biased variance) and, with groups == C and gamma == NULL, the
 * InstanceNorm1d/2d of the score heads (model/network.py:42-43).
 * cofi_group_stats writes stats (groups,2) = {mean, rstd}; deterministic two-level reduction,
 * combined in fp64.  ws: cofi_group_stats_workspace(M, C, groups, frames) bytes.
 * cofi_group_norm_apply:
 *   y = leaky( gn(x; stats, gamma, beta) + R , slope )   with
 *   R = 0                              if res == NULL
 *   R = res                            if res != NULL and res_stats == NULL
 *   R = gn(res; res_stats, rg, rb)     otherwise        (modules.py:222-240 residual tail)
 * slope = 1 is the identity, 0 is ReLU, 0.1 the reference's LeakyReLU.
 * The apply entry points read and write rows as float4: C, ldx, ldr, ldy multiples of 4 and >= C, x / res / y 16-byte aligned
 * (COFI_EINVAL otherwise).
 */
int cofi_group_stats_from_colpart(const float *colpart, int nslab, int M, int C, int groups, float eps, float *stats, int frames,
                                  cofi_stream_t stream);
int cofi_col_inv_norm_from_colpart(const float *colpart, int nslab, int M /* rows, all frames */, int ncols, int C, float eps, float *out,
                                   int frames, cofi_stream_t stream);
size_t cofi_group_stats_workspace(int M, int C, int groups, int frames);
int cofi_group_stats(const float *x, int ldx, int M, int C, int groups, float eps, float *stats /* (frames, groups, 2) */, void *ws,
                     size_t ws_bytes, int frames /* stack mode: M = frames * rows-per-frame, statistics per frame */, cofi_stream_t stream);
/* cofi_group_stats with every sum carried in fp64 (the training path: the backward of a normalisation amplifies a relative error of rstd
 * by the size of the component it removes; E[x^2] - mean^2 must not lose digits when |mean| >> std).  Same arguments, same workspace. */
int cofi_group_stats_exact(const float *x, int ldx, int M, int C, int groups, float eps, float *stats, void *ws, size_t ws_bytes, int frames,
                           cofi_stream_t stream);
int cofi_group_norm_apply(const float *x, int ldx, int M, int C, int groups, const float *stats, const float *gamma,
                          const float *beta, const float *res, int ldr, const float *res_stats, const float *res_gamma,
                          const float *res_beta, float slope, float *y, int ldy,
                          uint8_t *row_pos /* optional (M): row_pos[m] = (sum_c y[m,c] > 0), C <= 256 (kpconv.py:113-114) */, int frames, cofi_stream_t stream);

/* cofi_group_norm_apply with the statistics folded in-kernel from the producer's partials (cofi_norm_desc_t; `res_norm` = the
 * shortcut's own GroupNorm, same group count): no separate statistics launch.  row_pos (optional, M bytes):
 * row_pos[m] = (sum_c y[m,c] > 0), the per-row flag cofi_kpconv_aggregate takes (kpconv.py:113-114); needs C <= 256. */
/* Finalize a pending normalisation once, in a few workgroups: scale_shift (frames, 2, channels) as described at cofi_norm_desc_t.
 * Same fixed-order fp64 fold as the consumers' own: results do not depend on who folds. */
int cofi_norm_finalize(const cofi_norm_desc_t *norm, int rows, int frames, float *scale_shift, cofi_stream_t stream);
int cofi_group_norm_apply_partials(const float *x, int ldx, int M, int C, const cofi_norm_desc_t *norm, const float *res, int ldr,
                                   const cofi_norm_desc_t *res_norm, float *y, int ldy, uint8_t *row_pos, int frames,
                                   cofi_stream_t stream);
/* The two apply entry points emitting, in place of row_pos, the 16-byte support record of every row for the KPConv aggregation that
 * consumes y (cofi_kpconv_aggregate_rec): records[m] = (points[m], flag), flag = 1.0f where row_pos[m] would be 1.  points (M, 3),
 * records (M, 4) floats, 16-byte aligned; 16 <= C <= 256.  No extra launch, no extra pass. */
int cofi_group_norm_apply_rec(const float *x, int ldx, int M, int C, int groups, const float *stats, const float *gamma, const float *beta,
                              const float *res, int ldr, const float *res_stats, const float *res_gamma, const float *res_beta, float slope,
                              float *y, int ldy, const float *points, float *records, int frames, cofi_stream_t stream);
int cofi_group_norm_apply_partials_rec(const float *x, int ldx, int M, int C, const cofi_norm_desc_t *norm, const float *res, int ldr,
                                       const cofi_norm_desc_t *res_norm, float *y, int ldy, const float *points, float *records, int frames,
                                       cofi_stream_t stream);

/* Row LayerNorm: y = act(LN(x) * gamma + beta) (+ res).  Replaces nn.LayerNorm at
 * model/transformer/transformer.py:40-41,58,62 and model/network.py:29.  C <= 2048, C % 4 == 0; ldx / ldr / ldy multiples of 4
 * and >= C; x, res, y, gamma and beta 16-byte aligned (all are accessed as float4). */
/* cofi_layer_norm_act: the general form, y = leaky(LN(x) * gamma + beta + R1, slope) + R2 with R1 = res if res_first else 0 and
 * R2 = res otherwise; slope 1 = no activation, 0 = ReLU, 0.1 = the point encoder's LeakyReLU (the 'ln' configuration of
 * model/kpconv/modules.py:51-60: UnaryBlock / ConvBlock / the residual join of ResidualBlock). */
int cofi_layer_norm_act(const float *x, int ldx, int M, int C, const float *gamma, const float *beta, float eps, float slope, const float *res,
                        int ldr, int res_first, float *y, int ldy, cofi_stream_t stream);
int cofi_layer_norm(const float *x, int ldx, int M, int C, const float *gamma, const float *beta, float eps, int relu,
                    const float *res, int ldr, float *y, int ldy, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K6  flash-style multi-head attention on fp32 MFMA, never materialising the LxS score matrix.
 * Replaces model/transformer/linear_attention.py:56-79 (`FullAttention.forward`) together with
 * the per-channel query scaling of model/transformer/transformer.py:53
 * (F.normalize over the TOKEN axis): q'[l,c] = q[l,c] * q_colscale[c].
 *   O[l, h*D + d] = sum_s softmax_s( scale * <q'[l,h,:], k[s,h,:]> ) * v[s,h,d]
 * Q (frames*L, H*D) ldq; K,V (frames*S, H*D) ldk/ldv; O (frames*L, H*D) ldo.  D == 32.  q_colscale (frames, H*D) may be NULL.
 *
 * The work of a launch - (frame, head, 32-query block, 32-key block) units - is dealt out in equal contiguous ranges to about
 * one workgroup per CU whatever L, S and H are (one KITTI call is 160 query-block x head pairs of 40 units: whole pairs would
 * fill 160 of 256 CUs); a pair that is spread over several workgroups leaves one partial result per workgroup.
 *   cofi_attention_workspace  bytes of the partial-slot table `ws` (16-byte aligned device memory) for (L, S, H, frames)
 *   cofi_attention_parts      the attention kernel: fills `parts`.  Exactly one of q_colscale / q_colpart may be given;
 *                             q_colpart (q_nslab, q_ncols, 2) = the column partials of the projection that produced Q
 *                             (cofi_gemm_f32_colstats, Q = its first H*D columns; q_nslab = frames * ceil(L/64), L % 64 == 0
 *                             when frames > 1 - or the 32-row slabs cofi_loftr_tail writes: frames * ceil(L/32), L % 32 == 0): the token-axis norm of Q is then folded inside the kernel
 *   cofi_attention_merge      combines the slots of every query row into O (fixed order)
 *   cofi_attention_fwd, cofi_attention_fwd_colpart   = parts + merge
 * cofi_loftr_tail_parts_bf16x3 (K7) consumes `parts` directly: no merge launch, O never exists in memory.
 * cofi_col_inv_norm: out[c] = 1 / max(sqrt(sum_m x[m,c]^2), eps)  (F.normalize, eps 1e-12).
 */
size_t cofi_attention_workspace(int L, int S, int H, int D, int frames);
int cofi_attention_parts(const float *Q, int ldq, const float *K, int ldk, const float *V, int ldv, const float *q_colscale,
                         const float *q_colpart, int q_nslab, int q_ncols, float q_eps, int L, int S, int H, int D, float scale, int frames,
                         void *parts, size_t parts_bytes, cofi_stream_t stream);
/* the same kernel in the fp32-grade bf16 split arithmetic of cofi_gemm_* (bf16x3 = 2: K, V, scaled Q and the softmax weights cut into
 * three bf16 planes, six products per contraction on the bf16 matrix instruction, fp32 accumulation): same arguments, same slot table */
int cofi_attention_parts_bf16x6(const float *Q, int ldq, const float *K, int ldk, const float *V, int ldv, const float *q_colscale,
                                const float *q_colpart, int q_nslab, int q_ncols, float q_eps, int L, int S, int H, int D, float scale,
                                int frames, void *parts, size_t parts_bytes, cofi_stream_t stream);
/* The bf16x6 kernel with K / V split ONCE (round 6): cofi_attention_kv_planes cuts K and V (frames * S rows, H heads of 32 channels) into the
 * three bf16 planes of the split arithmetic, laid out per (frame, head, 32-key block) exactly as the attention kernel's LDS tiles
 * (K rows = keys; V transposed, keys in MFMA accumulator order; 12 288 bytes per block; rows past S are zero) - `planes`,
 * cofi_attention_kv_planes_bytes(S, H, D, frames) bytes, 16-byte aligned.  cofi_attention_parts_planes is cofi_attention_parts_bf16x6 reading
 * that image instead of K / V: same products in the same order, identical bits.  Without it every one of the L / 64 workgroups of a
 * (frame, head) repeats the split of the whole K / V. */
size_t cofi_attention_kv_planes_bytes(int S, int H, int D, int frames);
int cofi_attention_kv_planes(const float *K, int ldk, const float *V, int ldv, int S, int H, int D, int frames, void *planes, size_t planes_bytes,
                             cofi_stream_t stream);
int cofi_attention_parts_planes(const float *Q, int ldq, const void *planes, size_t planes_bytes, const float *q_colscale, const float *q_colpart,
                                int q_nslab, int q_ncols, float q_eps, int L, int S, int H, int D, float scale, int frames, void *parts,
                                size_t parts_bytes, cofi_stream_t stream);
int cofi_attention_merge(const void *parts, size_t parts_bytes, int L, int S, int H, int D, int frames, float *O, int ldo,
                         cofi_stream_t stream);
int cofi_attention_fwd(const float *Q, int ldq, const float *K, int ldk, const float *V, int ldv, const float *q_colscale,
                       float *O, int ldo, int L, int S, int H, int D, float scale, void *ws, size_t ws_bytes, int frames,
                       cofi_stream_t stream);
int cofi_attention_fwd_colpart(const float *Q, int ldq, const float *K, int ldk, const float *V, int ldv, const float *q_colpart,
                               int q_nslab, int q_ncols, float q_eps, float *O, int ldo, int L, int S, int H, int D, float scale,
                               void *ws, size_t ws_bytes, int frames, cofi_stream_t stream);
int cofi_col_inv_norm(const float *x, int ldx, int M, int C, float eps, float *out, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K6b  LoFTR linear attention, model/transformer/linear_attention.py:14-47 (`LinearAttention.forward`, no masks) with the token-axis
 * query scaling of transformer.py:53 (q' = q * q_colscale).  Per frame and head, phi(x) = elu(x) + 1:
 *   KV[d,v] = sum_s phi(k)[s,d] * (v[s,v] / S)     Ksum[d] = sum_s phi(k)[s,d]
 *   O[l, h*D + v] = (sum_d phi(q')[l,d] * KV[d,v]) * (1 / (sum_d phi(q')[l,d] * Ksum[d] + eps)) * S
 * Operands as for cofi_attention_parts: Q (frames*L, H*D) ldq; K, V (frames*S, H*D) ldk / ldv (column slices of a wider projection
 * buffer are fine: 16-byte aligned, leading dimensions multiples of 4); q_colscale (frames, H*D) or NULL; O (frames*L, H*D) ldo.  D == 32.
 * fp32 FMA throughout.  A summary launch over (128-row source chunk, head, frame) leaves one partial KV / Ksum per chunk in `ws`, a fold
 * launch sums them in a fixed order, an apply launch serves 64 query rows per workgroup: no floating-point atomics, the chunking depends on
 * S alone, so frame f of a stacked call has the bits of the single-frame call on its slice.  phi flushes exp() results below the smallest
 * normal number to zero: keys that are all very negative give O = 0 exactly.
 *   cofi_linear_attention_workspace  bytes of `ws` (16-byte aligned device memory); 0 = unsupported shape (D != 32)
 */
size_t cofi_linear_attention_workspace(int L, int S, int H, int D, int frames);
int cofi_linear_attention(const float *Q, int ldq, const float *K, int ldk, const float *V, int ldv, const float *q_colscale, int L, int S,
                          int H, int D, float eps, int frames, float *O, int ldo, void *ws, size_t ws_bytes, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K7  fused tail of one LoFTR encoder layer (d_model = 128), one kernel:
 *   out = x + LN2( relu([x | LN1(msg Wm^T)] W0^T) W2^T )         model/transformer/transformer.py:57-64
 * msg (L,128) ldm = attention output; x (L,128) ldx = layer input; weights PRE-SPLIT into bf16 hi/lo planes
 * ((N,K) row-major uint16 each: hi = bf16(w), lo = bf16(w - hi)); arithmetic = 3-term bf16 split with fp32
 * accumulation (as COFI_GEMM_BF16X3).  The intermediates never leave LDS. */
int cofi_loftr_tail_bf16x3(const float *msg, int ldm, const float *x, int ldx, const uint16_t *wm_hi, const uint16_t *wm_lo,
                           const float *n1_gamma, const float *n1_beta, const uint16_t *w0_hi, const uint16_t *w0_lo,
                           const uint16_t *w2_hi, const uint16_t *w2_lo, const float *n2_gamma, const float *n2_beta, float eps,
                           float *out, int ldo, int L, cofi_stream_t stream);
/* The same with msg still in the attention kernel's partial-slot form (cofi_attention_parts over (L, S, H, frames), H * 32 == 128):
 * the loader merges and normalises the slots of its rows; x / out hold frames * L rows. */
int cofi_loftr_tail_parts_bf16x3(const void *parts, size_t parts_bytes, int L, int S, int H, int frames, const float *x, int ldx,
                                 const uint16_t *wm_hi, const uint16_t *wm_lo, const float *n1_gamma, const float *n1_beta,
                                 const uint16_t *w0_hi, const uint16_t *w0_lo, const uint16_t *w2_hi, const uint16_t *w2_lo,
                                 const float *n2_gamma, const float *n2_beta, float eps, float *out, int ldo, cofi_stream_t stream);

/* The general form of K7 (both arithmetics, optional fused successors).  One launch computes the layer tail and, while the 32-row tile
 * of `out` is still in LDS, what the NEXT layers read first:
 *   proj s (s < 2, proj_n[s] in {0, 128, 256, 384}):  proj_y[s] (rows, proj_n[s]) = out @ proj_w[s]^T - stacked [Wq; Wk; Wv] blocks of
 *       the following layer(s) (model/transformer/transformer.py:45-47), weights pre-split like wm / w0 / w2; proj_part[s] (optional,
 *       (rows / 32, proj_n[s], 2)) = per 32-row slab and column {sum, sum of squares} of proj_y[s]: the table cofi_attention_parts
 *       takes as q_colpart (token-axis norm of Q, transformer.py:53); rows per frame % 32 == 0 then.
 *   out_l2 (rows, 128) ld_l2 and / or out_l2t (128, rows) ld_l2t (optional) = F.normalize(out, dim=1), token-major / channel-major
 *       (model/network.py:125-126 after the last layer).
 * planes = 2: COFI_GEMM_BF16X3 arithmetic, weights as (2, N, K) bf16 planes [hi | lo]; planes = 3: COFI_GEMM_BF16X6 (fp32-grade),
 * (3, N, K) planes [hi | mid | lo], hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid).  wm (p,128,128), w0 (p,256,256),
 * w2 (p,128,256), proj_w[s] (p, proj_n[s], 128).  Exactly one of msg (rows, 128) ldm / parts (cofi_attention_parts slot table over
 * (L, S, H, frames): rows = L * frames) is given. */
typedef struct cofi_loftr_tail_desc {
    const float *msg; int ldm; int rows;
    const void *parts; size_t parts_bytes; int L, S, H, frames;
    const float *x; int ldx;
    int planes;
    const uint16_t *wm, *w0, *w2;
    const float *n1_gamma, *n1_beta, *n2_gamma, *n2_beta;
    float eps;
    float *out; int ldo;
    int proj_n[2];
    const uint16_t *proj_w[2];
    float *proj_y[2]; int proj_ldy[2];
    float *proj_part[2];
    float *out_l2; int ld_l2;
    float *out_l2t; int ld_l2t;
    int w_frag;   /* 0: every weight plane is (N, K) row-major.  1: every plane is stored in MFMA-FRAGMENT ORDER - for row block T = n / 32 and
                   * k-step s = k / 16 the 64 x 8 bf16 a wave's B operand holds, lane-major:
                   *     plane[((T * (K / 16) + s) * 64 + lane) * 8 + i] = W[32 T + (lane & 31)][16 s + 8 (lane >> 5) + i]
                   * so that a wave's weight load is one contiguous 1 KB segment (row-major: 32 pieces of 32 B in 32 different lines). */
} cofi_loftr_tail_desc_t;
int cofi_loftr_tail(const cofi_loftr_tail_desc_t *desc, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K8 / glue.
 * cofi_pos_sine: model/transformer/position_encoding.py:29-50.  coords (T, n_dim) fp32 (or int32 grid
 * coordinates when coords_are_int), dim_t_host = the F frequencies (host array, F <= 64);
 * out[t, :] (+)= embedding, zero padded to d_model.  accumulate != 0 adds into `out`.
 * cofi_l2norm_rows: F.normalize(x, dim=1) of row-major rows (model/network.py:83-84,125-126):
 *   y[m,:] = x[m,:] / max(|x[m,:]|, 1e-12); if transpose != 0, y is written as (C, M) with ldy.
 * cofi_transpose: out (C,M) <- in (M,C).
 */
int cofi_pos_sine(const void *coords, int coords_are_int, int T, int n_dim, const float *dim_t_host, int F, int d_model,
                  int accumulate, float *out, int ldo, cofi_stream_t stream);
int cofi_l2norm_rows(const float *x, int ldx, int M, int C, float *y, int ldy, int transpose, cofi_stream_t stream);
/* the same rows into two destinations (y2 row-major, ldy2): the normalised 1/8 image map is both the transformer's input and the
 * up-sampler's (model/network.py:90,110,129) */
int cofi_l2norm_rows2(const float *x, int ldx, int M, int C, float *y, int ldy, float *y2, int ldy2, cofi_stream_t stream);
int cofi_transpose(const float *x, int ldx, int M, int C, float *y, int ldy, int frames /* x holds frames * M rows; y = frames blocks of (C, M) ldy */,
                   cofi_stream_t stream);
/* out (frames, C) = column means over the M / frames rows of each frame: nn.AdaptiveAvgPool2d(1) on an NHWC map
 * (model/imagenet.py:145,215). */
int cofi_col_mean(const float *x, int ldx, int M, int C, float *out, int frames, cofi_stream_t stream);
/* ---------------------------------------------------------------------------------------------
 * K13  image convolutions as implicit GEMM on the same MFMA kernel (no im2col buffer): x is an NHWC map
 * (H*W rows, ldx floats per pixel: a channel-concatenation is just a wider row), Wt is (Cout, ks*ks*Cin) with
 * k = (dy*ks + dx)*Cin + c, output y is NHWC (Ho*Wo, Cout).  ks in {1,3}, Cin % 4 == 0.
 *   y = act( conv(x) + bias + res )    and, if colpart != NULL, per-slab column statistics (InstanceNorm2d
 * statistics of model/imagenet.py:123 are per-channel = per-column; slab count / workspace as for
 * cofi_gemm_f32 with M = Ho*Wo, N = Cout, K = ks*ks*Cin).  Replaces nn.Conv2d of model/imagenet.py:25-33,
 * 137,380-395 (ResNet-34 trunk, ResidualConv).  `act` may carry COFI_GEMM_BF16X3.
 * cofi_im2col_stem: the 7x7/2 pad-3 stem convolution on the 3-channel NCHW image (imagenet.py:137) as
 *   an explicit (Ho*Wo, Kpad) matrix, k = (dy*7 + dx)*3 + c, zero padded to Kpad.
 * cofi_maxpool3x3s2_nhwc: nn.MaxPool2d(3, 2, 1) (imagenet.py:141).
 * cofi_upsample2x_cat_nhwc: bilinear x2 (align_corners=False) of `low` + channel concat with `skip`
 *   (imagenet.py:433,441-443), NHWC. */
int cofi_conv2d_nhwc(const float *x, int ldx, int H, int W, int Cin, const float *Wt, int Cout, int ks, int stride, int pad,
                     const float *bias, const float *res, int ldr, int act, float *y, int ldy, float *colpart, void *ws, size_t ws_bytes,
                     int frames, cofi_stream_t stream);
/* cofi_conv2d_nhwc with a pending normalisation of the INPUT map (x_norm, channels == Cin <= 512: the InstanceNorm + ReLU between
 * the two convolutions of a BasicBlock, imagenet.py:58-66; zero padding is applied after the normalisation, as nn.Conv2d pads the
 * normalised map) and a statistics table of width `stat_width`; see cofi_gemm_f32_fused.  `act` applies to the output columns
 * >= act_col0 only: two convolutions of ONE input - the skip branch and the first convolution of a ResidualConv, imagenet.py:397-403 -
 * run as one launch with the filters stacked [skip | conv1], act_col0 = the skip branch's channel count. */
int cofi_conv2d_nhwc_fused(const float *x, int ldx, const cofi_norm_desc_t *x_norm, int H, int W, int Cin, const float *Wt, int Cout, int ks,
                           int stride, int pad, const float *bias, const float *res, int ldr, int act, int act_col0, float *y, int ldy,
                           float *colpart, int stat_width, void *ws, size_t ws_bytes, int frames, cofi_stream_t stream);
int cofi_im2col_stem(const float *img_chw, int H, int W, int Kpad, float *out, int frames, cofi_stream_t stream);
int cofi_maxpool3x3s2_nhwc(const float *x, int H, int W, int C, float *y, int frames, cofi_stream_t stream);
int cofi_upsample2x_cat_nhwc(const float *low, int ldl, int C1, int h, int w, const float *skip, int lds, int C2, float *out, int ldo,
                             int frames, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K10-K12  coarse + fine matching without host round trips (model/network.py:145-161,167-226,
 * evaluation/eval_all.py:99-105).
 * cofi_row_argmin_1m: pix[n] = argmin_p (1 - sim[n,p]) with the lowest index on ties
 *   (network.py:176-180); sim (N,P) comes from cofi_gemm_f32 on the two descriptor sets.
 * cofi_select_matches: tries thresholds thr_host[0..n_thr) in order until at least `min_matches`
 *   super-points satisfy score >= thr AND 2 <= x <= x_max AND 2 <= y <= y_max (network.py:147-151; x = pix % W8,
 *   y = pix / W8; the reference hard-codes x_max = 62, y_max = 18 whatever the image size, network.py:184).  Writes (ascending point index) sel (cap N), coarse_xy (2, N) with
 *   leading dimension N, count_dev[0] = n, count_dev[1] = index of the threshold used (or -1).
 * cofi_extract_patches_nhwc: 4x4 windows [4*xy - 2, 4*xy + 2) of the NHWC map (H2*W2 rows of ldf floats) -> (n, C, 16)
 *   (network.py:206-226,156-158).
 * cofi_fine_match: cosine similarity of the 16 patch pixels against the point descriptor, argmax
 *   (first index on ties), fine_xy = 4*xy - 2 + (idx / 4, idx % 4)  [sic: x gets idx/4]
 *   (eval_all.py:99-105).  fine_xy (2, cap) with leading dimension `cap`.
 * cofi_fine_refine (no counterpart in the reference; declared behind cofi_match_finish, whose outputs it reads): the matched cell
 *   decoded geometrically - column idx % 4, row idx / 4 - plus a parabolic sub-pixel offset per axis from the similarities of its
 *   neighbours on the map.
 */
int cofi_row_argmin_1m(const float *sim, int lds, int N, int P, int32_t *pix, cofi_stream_t stream);
int cofi_select_matches(const float *score, const int32_t *pix, int N, int W8, int H8, int x_max, int y_max, const float *thr_host,
                        int n_thr, int min_matches, int32_t *sel, float *coarse_xy, int32_t *count_dev,
                        int frames /* stack mode: score / pix (frames, N), sel (frames, N), coarse_xy (frames, 2, N), count_dev (frames, 2) */,
                        cofi_stream_t stream);
int cofi_gather_points_sel(const float *pts, const int32_t *sel, const int32_t *count_dev, int cap, float *out,
                           cofi_stream_t stream);
int cofi_extract_patches_nhwc(const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                              const int32_t *count_dev, int cap, float *patches, cofi_stream_t stream);
int cofi_gather_rows_sel(const float *x, int ldx, int C, const int32_t *row_idx, const int32_t *count_dev, int cap, float *out,
                         int ldo, cofi_stream_t stream);
int cofi_fine_match(const float *patches, const float *pc_feats, int ldp, int C, const float *coarse_xy, int ldxy,
                    float center_scale, const int32_t *count_dev, int cap, float *fine_xy, int32_t *best, cofi_stream_t stream);
/* Everything that follows the match selection of a test-mode forward in ONE launch (model/network.py:153-161 + the caller's fine
 * matching, evaluation/eval_all.py:99-105): per accepted match i < count_dev[0] (sel[i] = its stage-4 point, coarse_xy[., i] its pixel)
 *   coarse_pts[i] = pts4[sel[i]];  node = point2node(pts1 (N1,3), that point) (network.py:250-264);  fine_pc[i] = fine_pc_all[node];
 *   patches[i] (C,16) = extract_patch(fmap (H2*W2, C) pixel-major, center_scale * xy) (network.py:206-226);  fine_xy / best = cofi_fine_match.
 * Bit-identical to cofi_gather_points_sel + cofi_nearest_node_sel + cofi_gather_rows_sel + cofi_extract_patches_nhwc + cofi_fine_match.
 * C <= 128; outputs sized at capacity `cap` (fine_xy (2, cap)). */
int cofi_match_finish(const float *pts4, const float *pts1, int N1, const int32_t *sel, const int32_t *count_dev, int cap,
                      const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                      const float *fine_pc_all, int ldfpc, float *coarse_pts, float *patches, float *fine_pc, int ldo,
                      float *fine_xy, int32_t *best, int N4 /* rows of pts4 per frame */,
                      int frames /* stack mode: every array holds `frames` equally sized blocks (coarse_xy (frames, 2, ldxy), count_dev (frames, 2)) */,
                      cofi_stream_t stream);
/* The same launch for a rig submission: frames = clouds x cameras images, image f looks at cloud f / cameras (the cameras of one cloud
 * are consecutive; frames % cameras == 0, else COFI_EINVAL).  pts4, pts1 and fine_pc_all - the three operands that belong to the cloud -
 * hold frames / cameras blocks; every other operand and every output is per image and laid out as cofi_match_finish lays it out.  Same
 * kernel: cofi_match_finish is this entry with cameras = 1. */
int cofi_match_finish_rig(const float *pts4, const float *pts1, int N1, const int32_t *sel, const int32_t *count_dev, int cap,
                          const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                          const float *fine_pc_all, int ldfpc, float *coarse_pts, float *patches, float *fine_pc, int ldo,
                          float *fine_xy, int32_t *best, int N4, int frames, int cameras, cofi_stream_t stream);
/* Sub-pixel refinement of the fine matches, behind cofi_match_finish.  Operands as that entry leaves them, in `frames`
 * equal blocks: fmap frames x H2*W2 rows of ldf floats, coarse_xy (frames, 2, ldxy) with ldxy >= cap, fine_pc (frames, cap, ldp) - the
 * per-match descriptor rows -, best (frames, cap), count_dev (frames, 2); outputs sub_xy (frames, 2, cap), peak (frames, cap).  Any
 * C >= 1.  Per match i < min(count_dev[2 f], cap), in fp32:
 *   px = floor(center_scale * x - 2) + best % 4, py = floor(center_scale * y - 2) + best / 4: the matched cell's column and row on the
 *     map.  This is the GEOMETRIC decode of best; fine_xy (cofi_fine_match) keeps the reference caller's transposed one.
 *   s(dx, dy) = cosine of map pixel (px + dx, py + dy) with fine_pc[i], each norm clamped at 1e-8; the channel sum runs in the same
 *     order for all five pixels, so equal vectors give bit-equal similarities.
 *   delta_x = 0 if px - 1 < 0 or px + 1 >= W2; else with den = (s(-1,0) - 2 s(0,0)) + s(1,0): den < 0 -> clamp(0.5 (s(-1,0) - s(1,0))
 *     / den, -0.5, 0.5), otherwise 0.5 sign(s(1,0) - s(-1,0)) (0 for equal neighbours and for NaN).  delta_y: the same with rows.
 *   sub_xy[0, i] = px + delta_x, sub_xy[1, i] = py + delta_y, peak[i] = s(0,0) (0 where that is not finite).
 *   Matched cell outside the map (a zero-padded patch cell won): both offsets 0 and peak 0.
 * With finite coarse_xy the outputs are finite whatever the map holds.  Rows i >= count_dev[2 f] are NOT written.  Frame f of a stacked
 * call is bit-identical to a single-frame call on its slice.  16-byte loads where fmap and fine_pc are 16-byte aligned and ldf and ldp
 * are multiples of 4; the results do not depend on it. */
int cofi_fine_refine(const float *fmap, int ldf, int C, int H2, int W2, const float *coarse_xy, int ldxy, float center_scale,
                     const float *fine_pc, int ldp, const int32_t *best, const int32_t *count_dev, int cap, float *sub_xy, float *peak,
                     int frames, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row f3, first part: the training losses of model/loss.py with their gradients w.r.t. the network outputs
 * (the backward of the network itself: second part, below).  grad_out = d(total)/d(loss), a device scalar; gradient
 * pointers may be NULL (forward only).  All fp32, fixed-order reductions (bit-reproducible).
 * cofi_desc_loss      loss.py:69-93: img / pc (C, K) with leading dimensions ldi / ldp (column = key point), mask (K, K);
 *                     -> loss[1], dists (K, K) = 1 - img^T pc (the reference returns it too); ws from cofi_desc_loss_workspace(K).
 * cofi_fine_circle_loss loss.py:9-51 (m = 0.2, gamma = 5 there): patches (K, C, 16), pc (K, C) rows of ldp, relative_index (K) int64
 *                     -> loss[1], per_kpt (K) scratch/output = log(1 + loss_n loss_p) per key point.
 * cofi_overlap_loss   loss.py:53-60: BCELoss(mean) of the in-picture scores against 1 and the out-of-picture scores against 0. */
size_t cofi_desc_loss_workspace(int K);
int cofi_desc_loss(const float *img, int ldi, const float *pc, int ldp, const float *mask, int C, int K, float pos_margin, float neg_margin,
                   float log_scale, float *loss, float *dists, const float *grad_out, float *grad_img, int ldgi, float *grad_pc, int ldgp,
                   void *ws, size_t ws_bytes, cofi_stream_t stream);
int cofi_fine_circle_loss(const float *patches, const float *pc, int ldp, const int64_t *relative_index, int K, int C, float m, float gamma,
                          float *loss, float *per_kpt, const float *grad_out, float *grad_patches, float *grad_pc, int ldg,
                          cofi_stream_t stream);
int cofi_overlap_loss(const float *inline_score, int n_in, const float *outline_score, int n_out, float *loss, const float *grad_out,
                      float *grad_in, float *grad_outline, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row f3, second part: the backward of the network (what torch.autograd derives for the reference's modules when train.py:285 calls
 * loss.backward()).  The dense contractions of the backward are cofi_gemm_f32* on transposed operands (cofi_transpose); these entry
 * points are the adjoints of the gathers.  A forward gather y[m] = f(x[idx[m, h]]) has the adjoint dx[j] = sum over the pairs (m, h)
 * with idx[m, h] == j: the caller passes the TRANSPOSED index table in CSR form - `pairs` = the ids m * H + h (for a row gather: m)
 * sorted by (j, id), `offsets` (N + 1) - and a wave per row j sums its list in that order: no float atomics, bit-reproducible.
 * cofi_kpconv_aggregate_bwd  model/kpconv/kpconv.py:91-105: dfeats[j, c] = sum_{(m,h)} sum_k w(m, h, k) dagg[m, k C + c] with the kernel-point
 *                            influences w recomputed from q_pts (M, 3), s_pts (N, 3), kernel_points (15, 3), sigma.  C >= 64 or a power of 2.
 * cofi_neighbor_maxpool_arg  functional.py:53-66 with the index h of the first neighbour attaining the maximum (arg (M, C) uint8);
 * cofi_neighbor_maxpool_bwd  its adjoint.   cofi_gather_rows_bwd: adjoint of cofi_gather_rows (functional.py:5-21).
 * cofi_im2col_nhwc / cofi_col2im_nhwc: a convolution of the image branch in training = im2col + GEMM (the weight gradient needs the
 *                            unfolded input): col (Ho Wo, ks ks C) with column (dy ks + dx) C + c; col2im is the adjoint (gather form).
 * cofi_attention_bwd         linear_attention.py:56-79, recompute style (no (L, S) matrix stored): q, k, v, o, d_o -> dq, dk, dv; exact fp32
 *                            matrix instruction; D == 32; ws of cofi_attention_bwd_workspace(L, H) bytes. */
int cofi_kpconv_aggregate_bwd(const float *dagg, int ldd, const float *q_pts, const float *s_pts, const int32_t *pairs, const int32_t *offsets,
                              int N, int C, int H, const float *kernel_points, float sigma, float *dfeats, int ldf, cofi_stream_t stream);
int cofi_neighbor_maxpool_arg(const float *x, int ldx, int N, int C, const int32_t *idx, int M, int H, float *out, int ldo,
                              uint8_t *arg /* (M, C) bytes; H <= 256, C % 4 == 0 */, cofi_stream_t stream);
int cofi_neighbor_maxpool_bwd(const float *dy, int ldy, const uint8_t *arg, int C, int H, const int32_t *pairs, const int32_t *offsets, int N,
                              float *dx, int ldx, cofi_stream_t stream);
int cofi_gather_rows_bwd(const float *dy, int ldy, int C, const int32_t *pairs, const int32_t *offsets, int N, float *dx, int ldx,
                         cofi_stream_t stream);
int cofi_im2col_nhwc(const float *x, int ldx, int H, int W, int C, int ks, int stride, int pad, float *col, int ldc, cofi_stream_t stream);
int cofi_col2im_nhwc(const float *dcol, int ldc, int H, int W, int C, int ks, int stride, int pad, float *dx, int ldx, cofi_stream_t stream);
/* Backward of y = leaky(gn(x; stats) * gamma + beta + res, slope) (cofi_group_stats + cofi_group_norm_apply: GroupNorm over all rows,
 * InstanceNorm with groups == C, train-mode BatchNorm): dx, dgamma, dbeta (either may be NULL), dres (NULL without a residual) from
 * x, y (the forward's output: its sign selects the activation slope; unused for slope == 1), dy and the forward's stats (groups, 2).
 * const_stats != 0: the statistics were constants (eval-mode BatchNorm on running statistics).  Channels per group: a power of two <= 64.
 * Three fixed-order stages; ws of cofi_group_norm_bwd_workspace(M, C, groups) bytes. */
size_t cofi_group_norm_bwd_workspace(int M, int C, int groups);
int cofi_group_norm_bwd(const float *x, int ldx, const float *y, int ldy, const float *dy, int lddy, int M, int C, int groups, const float *stats,
                        const float *gamma, float slope, int const_stats, float *dx, int lddx, float *dgamma, float *dbeta, float *dres, int lddr,
                        void *ws, size_t ws_bytes, cofi_stream_t stream);
size_t cofi_col_sum_workspace(int M, int C);   /* out[c] = sum_m x[m, c] (bias gradients), two fixed-order stages */
int cofi_col_sum(const float *x, int ldx, int M, int C, float *out, void *ws, size_t ws_bytes, cofi_stream_t stream);

/* F.normalize(x, dim=0) of a (M, C) matrix (model/transformer/transformer.py:53: Q is normalised over the tokens), forward and backward.
 * bwd == 0: out = y, stats (2, C) = 1 / max(norm, eps) | (norm >= eps) written.  bwd != 0: out = dx for the upstream gradient dy, stats read.
 * Two launches per call, every sum in a fixed order. */
/* backward of cofi_l2norm_rows (F.normalize(x, dim=1), network.py:83-84, 90, 125-126): dx for the upstream gradient dy, eps = 1e-12 */
int cofi_l2norm_rows_bwd(const float *x, int ldx, const float *dy, int lddy, int M, int C, float eps, float *dx, int lddx, cofi_stream_t stream);
/* adjoint of the bilinear x2 up-sampling of cofi_upsample2x_cat_nhwc (imagenet.py:433): dout = the gradient of the (2h 2w, C1 + C2) map, of which the
 * first C1 columns are read; dlow (h w, C1).  Gather form per input pixel: no atomics, fixed order. */
int cofi_upsample2x_bwd_nhwc(const float *dout, int lddo, int C1, int h, int w, float *dlow, int lddl, cofi_stream_t stream);
/* y1 = x1^T, y2 = x2^T for two matrices of M rows (x1 (M, C1), x2 (M, C2)) in one launch - dW = dY^T X of a linear layer needs both */
int cofi_transpose_pair(const float *x1, int ldx1, int C1, float *y1, int ldy1, const float *x2, int ldx2, int C2, float *y2, int ldy2, int M,
                        cofi_stream_t stream);
size_t cofi_col_normalize_workspace(int M, int C);
int cofi_col_normalize(const float *x, int ldx, const float *dy, int lddy, int M, int C, float eps, int bwd, float *stats, float *out, int ldo,
                       void *ws, size_t ws_bytes, cofi_stream_t stream);
size_t cofi_attention_bwd_workspace(int L, int H);
int cofi_attention_bwd(const float *q, int ldq, const float *k, int ldk, const float *v, int ldv, const float *o, int ldo, const float *d_o,
                       int lddo, int L, int S, int H, int D, float scale, float *dq, int lddq, float *dk, int lddk, float *dv, int lddv, void *ws,
                       size_t ws_bytes, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row f1: camera pose from the fine matches, replacing the reference's
 *   cv2.solvePnPRansac(cameraMatrix=K, imagePoints=fine_xy.T, objectPoints=coarse_pc_points, iterationsCount=10000,
 *                      distCoeffs=None)                                   (evaluation/eval_all.py:107)
 * = RANSAC over minimal-set hypotheses scored by reprojection error (threshold `reproj_err`, OpenCV default 8 px), best
 * consensus set, Levenberg-Marquardt refit on its inliers.  Here: `iterations` P3P hypotheses evaluated in parallel (4 sampled
 * correspondences each; counter-based sampling from `seed`, reproducible), winner = most inliers (lowest id on ties), LM refit
 * (`refine_iters` steps) in one workgroup.  Everything stays on the device: obj (n,3), img (n,2) are read up to
 * count_dev[0] rows (or n_max if count_dev == NULL).  Outputs: pose[12] = R row-major | t with x_cam = R X + t;
 * result[3] = {success, inliers of the RANSAC model, winning hypothesis id}; inlier_mask (n_max bytes).
 * OpenCV is absent from this image: parity with it is unpinned; oracle/pnp_oracle.py is the restatement it is tested against. */
size_t cofi_pnp_ransac_workspace(int iterations);
int cofi_pnp_ransac(const float *obj, const float *img, const int32_t *count_dev, int n_max, float fx, float fy, float cx, float cy,
                    int iterations, float reproj_err, unsigned seed, int refine_iters, void *ws, size_t ws_bytes, float *pose,
                    int32_t *result, uint8_t *inlier_mask, cofi_stream_t stream);
/* The same solver for `frames` frames of a stack-mode submission in two launches (hypotheses + consensus with the frame on the grid's
 * second axis, one refit workgroup per frame).  Frame f is bit-identical to cofi_pnp_ransac on that frame's operands with seed + f: both
 * forms run the same device functions.  Operands are addressed in place, as the stack-mode forward leaves them:
 *   obj    frame f at obj + f * obj_frame_stride floats, (n_max, 3)
 *   img    frame f at img + f * img_frame_stride floats; point-major (n_max, 2), or coordinate-major (2, n_max) if coord_major != 0
 *          (the fine_xy of cofi_match_finish)
 *   count_dev[f * count_stride] = valid rows of frame f (NULL: n_max for every frame); fewer than 4: result {0, 0, -1}, identity pose
 *   K_dev  (frames, 3, 3) float32 row-major in DEVICE memory: fx, fy, cx, cy are read by the kernels (no host copy of the intrinsics);
 *          a frame whose fx or fy is not positive reports failure
 * Outputs: pose (frames, 12), result (frames, 3), inlier_mask (frames, n_max).  Workspace: one key per frame + iterations x 12 floats
 * per frame.  The hypotheses kernel stages a frame's correspondences in LDS (20 bytes each) when n_max <= 3276, and reads global
 * memory beyond. */
size_t cofi_pnp_ransac_batch_workspace(int iterations, int frames);
int cofi_pnp_ransac_batch(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                          const int32_t *count_dev, int count_stride, const float *K_dev, int n_max, int frames, int iterations,
                          float reproj_err, unsigned seed, int refine_iters, void *ws, size_t ws_bytes, float *pose, int32_t *result,
                          uint8_t *inlier_mask, cofi_stream_t stream);
/* ONE pose per rig: the `cameras` = C images of a rig are bolted to one body, and the solver finds the pose of that body (rig <- cloud)
 * from the matches of all its cameras.  The operands are those of cofi_pnp_ransac_batch for rigs * C frames, image f = s * C + c being
 * camera c of rig s (the layout of a rig submission), plus
 *   ext_dev  extrinsics in DEVICE memory, 12 floats per camera [R row-major | t], camera <- rig: Y_cam = R_c Y_rig + t_c; camera c of
 *            rig s at ext_dev + s * ext_rig_stride + 12 c.  ext_rig_stride 0: one set of C shared by all rigs; >= 12 C: one per rig.
 * Rig s uses seed + s.  A camera is usable if fx > 0 and fy > 0, eligible if usable with >= 4 rows.  Hypothesis h draws an eligible
 * camera in proportion to its rows (hash j = 4), four rows of it as the batched solver does (at C = 1: the same samples), solves P3P
 * there and carries the pose into the rig frame, T = E_c^-1 o pose_c (fp64, rounded once into the slab).  It is scored over every
 * usable camera with >= 1 row through E_c o T (fp64, rounded once) and the batched solver's inlier test; most inliers in total win,
 * lowest id on ties.  One workgroup per rig refits T on all cameras' inliers (LM, left-multiplied increments on T).  A rig without an
 * eligible camera fails even if its rows add up to 4 or more: no minimal solver across cameras (generalised P3P) is included.
 * Outputs: rig_pose (rigs, 12), rig_result (rigs, 3) = {success, inliers of all cameras, hypothesis}; per image pose (rigs C, 12) =
 * E_c o rig_pose (fp64, rounded once), result (rigs C, 3) = {rig success, this image's inliers, hypothesis}, inlier_mask (rigs C, n_max).
 * A failed rig: {0, 0, -1} and identity poses for the rig and all its images, zero masks.  Workspace: one key and one slab of
 * iterations x 12 floats per RIG (the slab holds rig poses).  The hypotheses kernel stages ONE camera's rows at a time in LDS when
 * n_max <= 3276 (the batched kernel's footprint whatever C is) and reads global memory beyond: chosen by n_max alone.  A memset and
 * two launches on `stream`, no host synchronisation.  rigs * cameras <= 65535. */
size_t cofi_pnp_ransac_rig_workspace(int iterations, int rigs);
int cofi_pnp_ransac_rig(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                        const int32_t *count_dev, int count_stride, const float *K_dev, const float *ext_dev, int ext_rig_stride, int n_max,
                        int cameras, int rigs, int iterations, float reproj_err, unsigned seed, int refine_iters, void *ws, size_t ws_bytes,
                        float *rig_pose, int32_t *rig_result, float *pose, int32_t *result, uint8_t *inlier_mask, cofi_stream_t stream);
/* The registration errors of evaluation/eval_all.py:16-22 for `frames` poses: P_diff = inv(P_pred) P_gt (general fp64 inverse),
 * out (frames, 2) float64 = [RTE = |t(P_diff)|, RRE = sum |euler 'xzy' of R(P_diff)| in degrees, scipy's gimbal convention].
 * pose (frames, 12) as cofi_pnp_ransac writes it; P_gt (frames, 4, 4) row-major, float64 if gt_is_f64 != 0, else float32. */
int cofi_pose_errors(const float *pose, const void *P_gt, int gt_is_f64, int frames, double *out, cofi_stream_t stream);
/* Pose uncertainty: the 6 x 6 Gauss-Newton covariance of the refit's least-squares problem at the pose cofi_pnp_ransac returned, over
 * the consensus set it wrote into inlier_mask.  obj, img, count_dev, n_max and the intrinsics are that call's operands; pose (12),
 * result (3) and inlier_mask (n_max) its outputs, read only.  Tangent vector delta = (omega, v), rotation first (radians, then the
 * units of obj), of the left-multiplied perturbation R' = exp(omega) R, t' = exp(omega) t + v; residual = projected - observed, pixels.
 *   rows used   i < count, inlier_mask[i] != 0, depth under the pose > 1e-6 (fp64); n of them
 *   H = sum J_i^T J_i, cost = sum |r_i|^2 in fp64, J_i the 2 x 6 Jacobian of the refit
 *   sigma_hat^2 = cost / (2 n - 6);  sigma^2 = sigma_px^2 if sigma_px > 0, else sigma_hat^2
 *   info = H / sigma^2, cov = sigma^2 H^-1 through the Cholesky factorisation of D^-1/2 H D^-1/2, D = diag(H); min_pivot = the
 *   smallest squared diagonal entry of the factor, in (0, 1]
 * Outputs in DEVICE memory, float64: cov (36), info (36) row-major and exactly symmetric, stat (4) = {ok, n, sigma_hat^2 (0 where
 * 2 n - 6 <= 0), min_pivot}.  ok = 0 with all-zero matrices and min_pivot 0 - never NaN or Inf - when result[0] == 0, 2 n - 6 <= 0
 * (sigma estimated), sigma^2 is not > 0, a diagonal entry of H is not > 0, a pivot is <= 1e-12, or any accumulated or resulting value
 * is not finite.  One launch of one wave; results are bit-reproducible.  COFI_EINVAL: a NULL operand, n_max <= 0, fx or fy not
 * positive, sigma_px NaN.  It is NOT a model of outliers inside the gate or of the choice of the consensus set. */
int cofi_pose_covariance(const float *obj, const float *img, const int32_t *count_dev, int n_max, float fx, float fy, float cx, float cy,
                         const float *pose, const int32_t *result, const uint8_t *inlier_mask, float sigma_px, double *cov, double *info,
                         double *stat, cofi_stream_t stream);
/* The same for the `frames` frames of cofi_pnp_ransac_batch in one launch (one wave per frame): the operands up to `frames` are read
 * exactly as that call reads them, pose (frames, 12), result (frames, 3), inlier_mask (frames, n_max) are its outputs.  cov, info
 * (frames, 36), stat (frames, 4).  A frame whose fx or fy is not positive has ok = 0.  Frame f is bit-identical to
 * cofi_pose_covariance on that frame's operands. */
int cofi_pose_covariance_batch(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                               const int32_t *count_dev, int count_stride, const float *K_dev, int n_max, int frames, const float *pose,
                               const int32_t *result, const uint8_t *inlier_mask, float sigma_px, double *cov, double *info, double *stat,
                               cofi_stream_t stream);
/* One covariance per RIG, in the rig's tangent space (perturbations of rig <- cloud): the operands of cofi_pnp_ransac_rig up to `rigs`,
 * its rig_pose (rigs, 12) and rig_result (rigs, 3), and its per-image inlier_mask (rigs C, n_max).  Rows of every camera with usable
 * intrinsics enter, camera-major, with the rig refit's Jacobian d(pi)/dY_c . R_c . [-[Y_rig]x | I]; a rig none of whose cameras is
 * usable has ok = 0.  cov, info (rigs, 36), stat (rigs, 4).  The covariance of camera c's pose E_c o T follows by the adjoint of E_c. */
int cofi_pose_covariance_rig(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                             const int32_t *count_dev, int count_stride, const float *K_dev, const float *ext_dev, int ext_rig_stride,
                             int n_max, int cameras, int rigs, const float *rig_pose, const int32_t *rig_result, const uint8_t *inlier_mask,
                             float sigma_px, double *cov, double *info, double *stat, cofi_stream_t stream);
/* Normalised estimation error squared of `frames` poses against ground truth: omega = log(R_gt R_est^T), v = t_gt - exp(omega) t_est,
 * e = (omega, v), nees = e^T info e; NaN where stat[4 f] == 0.  pose (frames, 12); P_gt (frames, 4, 4) row-major in the direction of
 * the pose, float64 if gt_is_f64 != 0, else float32; info (frames, 36), stat (frames, 4) as cofi_pose_covariance* write them; nees
 * (frames) float64.  One thread per pose. */
int cofi_pose_nees(const float *pose, const void *P_gt, int gt_is_f64, const double *info, const double *stat, int frames, double *nees,
                   cofi_stream_t stream);
/* The evaluation pass (evaluation/eval_all.py:107-117 and evaluation/IR_RMSE.py:36-59) for the `frames` frames of a stack-mode
 * submission, behind cofi_pnp_ransac_batch: one launch, one 256-thread workgroup per frame, no host read.  obj, img, count_dev, K_dev,
 * n_max and their strides are those of cofi_pnp_ransac_batch (a negative count is read as 0); pose (frames, 12) and result (frames, 3)
 * are that call's outputs; P_gt (frames, 4, 4) row-major, float64 if gt_is_f64 != 0, else float32 (the GT_P of the reference: x_cam =
 * R_gt x + t_gt); thresholds (T) float64 in DEVICE memory, 1 <= T <= 64 (COFI_EUNSUPPORTED beyond), in any order; row_index (frames)
 * int32; rows (table_rows, 6 + T) float64.  Frame f writes row row_index[f] of the table and nothing else; an index that is negative
 * (the padding frames of a flushed stack) or not below table_rows makes the frame leave at once.  The columns of a row:
 *   0       n        valid correspondences of the frame
 *   1, 2    success, inliers = result[f, 0], result[f, 1]
 *   3, 4    RTE, RRE of cofi_pose_errors (the same device function) for this frame's pose; NaN when success == 0
 *   5       the mean of residual_i = |img_i - gt_pixel_i|, gt_pixel = proj[0:2] / proj[2], proj = K (R_gt x_i + t_gt)  (IR_RMSE.py:58, the
 *           reference's "RMSE"); NaN when n == 0
 *   6 + i   the number of residuals <= thresholds[i] (IR_RMSE.py:59 before the division); 0 when n == 0
 * All arithmetic is fp64; the residual sum is taken in an order that depends on n only, so a frame's row is bit-identical in any batch
 * and at any position.  A point behind the camera is not special: a NaN residual compares false and makes the mean NaN. */
int cofi_eval_monitors(const float *obj, int obj_frame_stride, const float *img, int img_frame_stride, int coord_major,
                       const int32_t *count_dev, int count_stride, const float *K_dev, int n_max, int frames, const float *pose,
                       const int32_t *result, const void *P_gt, int gt_is_f64, const double *thresholds, int T, const int32_t *row_index,
                       double *rows, int table_rows, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The validation pass of train.py (test_acc, train.py:27-106; fine_recall, :271-281; the pc_score scalars, :256-259) for the `frames`
 * frames of a stack-mode mode='val' submission, with no host read.  Label tensors are device tensors, all int64 (idx_is_i64 != 0) or all
 * int32, laid out (frames, K) - index lists, frame-local - or (frames, 2, K) - pixel coordinates, x row first.
 *
 * cofi_val_gather: the label gathers of network.py:137-141 for every frame in one launch.
 *   patches (frames, K, C, 16) = extract_patch(fmap of frame f (H2*W2, C) pixel-major, centers[f]) (network.py:206-226; zero outside the map),
 *   fine_pc (frames, K, C)     = row inline_idx[f, k] of frame f's fine point descriptors fine_pc_map (frames * N1, ldfpc) (zero row for an
 *   index outside [0, N1)).
 *
 * cofi_val_monitors: per frame f, reading the forward's outputs in place - img_desc (frames, C, T) and pc_desc (frames, C, N4)
 * channel-major coarse descriptors (T = H8 * W8 pixels of a W8 wide map), points4 (frames * N4, 3), pc_score (frames * N4),
 * patches / fine_pc as cofi_val_gather writes them, K_4 (frames, 3, 3), P (frames, 4, 4) -
 *   img_i / pc_j   = the descriptor columns coarse_img_kpt_idx[f, i] / pc_kpt_idx[f, j]                              (train.py:72-78)
 *   pc_xy_j        = proj[:2] / proj[2], proj = K_4 (P[:3,:3] x_j + P[:3,3])                                          (train.py:80-82)
 *   mask[i, j]     = sqrt(|img_xy_i - pc_xy_j|^2) <= dist_thres, img_xy = (index % W8, index / W8)                    (train.py:84)
 *   dist[i, j]     = 1 - <img_i, pc_j>, one fp32 fmaf chain over the channels in ascending order                       (train.py:86)
 *   n_true[f]      = the number of entries with mask set and dist != 0: the reference's true_value_list                (train.py:89-91)
 *   counts[f, k-1] = over all rows, how many of the row's k smallest dist values (ascending, torch.sort) EQUAL ANY VALUE of the
 *                    true list - membership by value over the whole matrix, not by position, as `candidate in true_value_list`
 *                    (train.py:92-101); counts (frames, topk), topk <= 8 and <= K
 *   fine_hits[f]   = key points whose arg-max over the 16 patch pixels of the cosine similarity with fine_pc (cofi_fine_match's
 *                    arithmetic and first-index tie rule) equals (fine_xy - fine_center_kpt_coors + 2) folded as y * 4 + x  (train.py:268-279)
 *   score_stats[f] = [max, min, mean] of pc_score at pc_kpt_idx[f], then at pc_outline_idx[f]                            (train.py:256-259)
 * dist_out / mask_out (frames, K, K) fp32, optional (NULL to skip): the distance matrix and the mask (1 / 0) the counts come from.
 * One launch: workgroup (f, 0) holds the distance tile and the true-value list in LDS, workgroup (f, 1) the fine and score part.
 * K <= 128 and C <= 128 (what fits the LDS of one workgroup); COFI_EUNSUPPORTED beyond.  Label indices outside their table are clamped
 * into it.  The workspace is empty (the query returns 0); ws may be NULL. */
int cofi_val_gather(const float *fmap, int ldf, int C, int H2, int W2, const float *fine_pc_map, int ldfpc, int N1, const void *centers,
                    const void *inline_idx, int idx_is_i64, int K, int frames, float *patches, float *fine_pc, cofi_stream_t stream);
size_t cofi_val_monitors_workspace(int K, int frames);
int cofi_val_monitors(const float *img_desc, const float *pc_desc, int C, int T, int W8, int N4, const float *points4,
                      const float *pc_score, const float *patches, const float *fine_pc, int C2, const void *pc_kpt_idx,
                      const void *pc_outline_idx, const void *coarse_img_kpt_idx, const void *fine_xy, const void *fine_center_kpt_coors,
                      int idx_is_i64, const float *K_4, const float *P, float dist_thres, int K, int frames, int topk, int32_t *counts,
                      int32_t *n_true, int32_t *fine_hits, float *score_stats, float *dist_out, float *mask_out, void *ws,
                      size_t ws_bytes, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row f2: the data side of one frame on the device, replacing the numpy / open3d / cv2 part of
 *   kitti_pc_img_dataset.__getitem__                                        (data/kitti.py:259-393)
 * between the disk read and the model call.  The random draws (choice indices, SE(3), permutations) are made on the host in the
 * reference's call order (cofii2p_amd/dataside.py: FrameSampler) and handed in as plain arrays; the coarse / fine label
 * projection works on 1280 points and stays host-side numpy.
 *   cofi_pack_transform_scan  data7n (7, N) channel-major [xyz | intensity | normal] (the on-disk layout) -> rows8 (N, 8) =
 *       [T p | intensity | R n | 0], T = 4x4 row-major in device memory (P_cam * Tr, kitti.py:273-277)
 *   cofi_voxel_downsample     open3d voxel_down_sample(voxel) of points + colours(intensity / max) + normals (kitti.py:145-166):
 *       voxel index = floor((p - (min_bound - voxel / 2)) / voxel), double-precision means per voxel, out_rows8 (cap, 8) in ascending
 *       (ix, iy, iz) order (open3d's order is that of an unordered_map: parity with it is unpinned), count_dev[0] = voxels,
 *       count_dev[1] = 1 if an index overflowed 13 bits.  Stable radix sort + segmented means: bit-reproducible.
 *   cofi_gather_transform     rows choice[i] (kitti.py:168-180), x' = R x + t, n' = R n (kitti.py:284-288), feats = [intensity | n']
 *       (kitti.py:293): points (n, 3), feats (n, 4)
 *   cofi_resize_crop_image    cv2.resize(INTER_LINEAR) of the uint8 HWC image to (dst_h, dst_w) in OpenCV's 11-bit fixed point, crop
 *       [crop_y, crop_y + H) x [crop_x, crop_x + W), / 255, HWC -> CHW (kitti.py:306-322, 375).  cv2 is absent from this image:
 *       parity with it is unpinned. */
/*   cofi_color_jitter_chw     train mode (kitti.py:193-201,329-330): torchvision ColorJitter on the cropped image = the four operations of its
 *       PIL path in the order `order4` (host array: 0 brightness, 1 contrast, 2 saturation, 3 hue) with the given factors, applied in
 *       place to the (3, H, W) float image cofi_resize_crop_image wrote (values k / 255).  Bit-equal to PIL.ImageEnhance / PIL's HSV
 *       conversions (torchvision itself is absent: its published algorithm; PIL is present and pins the restatement).  ws: 8 bytes. */
int cofi_color_jitter_chw(float *img, int H, int W, const int *order4, float brightness, float contrast, float saturation, float hue, void *ws,
                          size_t ws_bytes, cofi_stream_t stream);
int cofi_pack_transform_scan(const float *data7n, int N, const float *P44_dev, float *rows8, cofi_stream_t stream);
size_t cofi_voxel_downsample_workspace(int N);
int cofi_voxel_downsample(const float *rows8, int N, double voxel, float *out_rows8, int cap, int32_t *count_dev, void *ws, size_t ws_bytes,
                          cofi_stream_t stream);
/* The two neighbourhood operators north_star names, model/kpconv/ops/grid_subsample.py and radius_search.py.  In the reference both
 * call an extension that is not vendored (geotransformer.ext) and nothing on the forward path uses them; built here on the kernels
 * above, parity with the extension unpinned (restated from the published KPConv / GeoTransformer C++):
 *   cofi_grid_subsample  barycentre of every occupied cell of a `voxel` grid with origin floor(min / voxel) * voxel, float32 arithmetic in
 *       input order, output (count, 3) in ascending (iz, iy, ix) order; ONE batch element per call; ws = cofi_voxel_downsample_workspace(N)
 *   cofi_radius_mask     sorted k-nearest rows (cofi_knn_topk*: idx (M,k) into S support rows, squared distances) -> int64 rows in which
 *       slots at squared distance >= radius^2 (or past the support) hold `fill`, the others idx + offset; max_count_dev[0] (zeroed by the
 *       caller) = the largest number of neighbours kept in a row (the extension's output width) */
int cofi_grid_subsample(const float *points, int N, float voxel, float *out_points, int cap, int32_t *count_dev, void *ws, size_t ws_bytes,
                        cofi_stream_t stream);
int cofi_radius_mask(const int32_t *idx, const float *dist, int M, int k, int S, float radius, long long offset, long long fill, long long *out,
                     int32_t *max_count_dev, cofi_stream_t stream);
int cofi_gather_transform(const float *vox_rows, const int32_t *choice, int n, const float *P44_dev, float *points, float *feats,
                          int feats_are_points /* 0: feats = [intensity | R n] (kitti.py:293); 1: [intensity | R x + t] (nuscenes.py:204) */,
                          cofi_stream_t stream);
int cofi_resize_crop_image(const uint8_t *src_hwc, int src_h, int src_w, int dst_h, int dst_w, int crop_y, int crop_x, int H, int W,
                           float *out_chw, cofi_stream_t stream);
/* Raw nuScenes sweeps -> the stored sample FramePreparer(dataset='nuscenes') takes (data/build_nuscenes/build_dataset.py:41-54, 109-185,
 * 217-300; cofii2p_amd/sweeps.py).  Every floating-point result is a chain of separate correctly rounded products and sums in the stated
 * order (no contraction), so tests/sweeps_refs.py restates it bit for bit; parity with open3d, cv2 and pyquaternion is unpinned.
 *   cofi_accumulate_sweeps   rows (total_rows, ld) float32, ld = 5 (.pcd.bin: x y z intensity ring) or 4: the S <= 64 sweeps back to back,
 *       sweep j at rows offsets_dev[j] .. offsets_dev[j + 1] (S + 1 int32 in device memory, offsets[0] = 0, offsets[S] = total_rows, empty
 *       sweeps allowed); T_dev (S, 4, 4) float64 row-major, sweep j -> key sweep (entry 0 is not read).  A row is dropped iff
 *       (x < 0.8f) & (x > -0.8f) & (y < 2.7f) & (y > -2.7f) in its own frame (:115-121); the others come out in input order (stable
 *       compaction: chunk counts, scan, ordered writes - no float atomics): points (total_rows, 3) float64 = the widened row for sweep 0,
 *       s = T[a][0] * x; s = s + T[a][1] * y; s = s + T[a][2] * z; s = s + T[a][3] in double for the others; intensity (total_rows) float32;
 *       count_dev[0] = rows kept.  ws = cofi_accumulate_sweeps_workspace(total_rows), 16-byte aligned.
 *   cofi_voxel_downsample_f64  cofi_voxel_downsample on float64 points (N, 3) + float32 intensity (N): the voxel index is taken from the
 *       float64 point (not from its float32 rounding), means in double in input order times 1.0 / count, out_rows4 (cap, 4) float32 =
 *       [float32(mean) | float32(mean(float32(intensity / max)) * (double)max)] (:52 multiplies in double, :227 casts afterwards) in
 *       ascending (ix, iy, iz) order; count_dev[0] = voxels (may exceed cap: the first cap rows are written), count_dev[1] = 1 if an index
 *       overflowed 13 bits.  ws = cofi_voxel_downsample_f64_workspace(N), 16-byte aligned; out_rows4 16-byte aligned.
 *   cofi_sweeps_to_camera    rows4 (M, 4) -> out_4m (4, M) float32 channel-major = [float32(c) | intensity], c = R p + t with P44_dev the
 *       float64 4x4 P_cam_pc and p widened, s = R[a][0] * x; s = s + R[a][1] * y; s = s + R[a][2] * z; s = s + t[a]; uvz = K c with K33_dev
 *       float32 widened, same order, no translation.  inside_dev[0] (zeroed by the call, integer atomics) = rows with uvz[2] > 0 and
 *       0 <= uvz[0] / uvz[2] <= W - 1 and 0 <= uvz[1] / uvz[2] <= H - 1 (:270-280).
 *   cofi_resize_image_u8     rows [top_rows, src_h) of the uint8 HWC image through cv2.resize(INTER_LINEAR) to (dst_h, dst_w), the fixed-point
 *       arithmetic of cofi_resize_crop_image, stored as uint8 HWC (:252-260).
 * COFI_EINVAL: NULL or misaligned operand, ld not 4 or 5, S outside 1..64, non-positive sizes, top_rows outside [0, src_h);
 * COFI_EWORKSPACE: ws NULL, misaligned or too small. */
size_t cofi_accumulate_sweeps_workspace(int total_rows);
int cofi_accumulate_sweeps(const float *rows, int ld, const int32_t *offsets_dev, int S, int total_rows, const double *T_dev, double *points,
                           float *intensity, int32_t *count_dev, void *ws, size_t ws_bytes, cofi_stream_t stream);
size_t cofi_voxel_downsample_f64_workspace(int N);
int cofi_voxel_downsample_f64(const double *points, const float *intensity, int N, double voxel, float *out_rows4, int cap, int32_t *count_dev,
                              void *ws, size_t ws_bytes, cofi_stream_t stream);
int cofi_sweeps_to_camera(const float *rows4, int M, const double *P44_dev, const float *K33_dev, int H, int W, float *out_4m,
                          int32_t *inside_dev, cofi_stream_t stream);
int cofi_resize_image_u8(const uint8_t *src_hwc, int src_h, int src_w, int top_rows, int dst_h, int dst_w, uint8_t *dst_hwc,
                         cofi_stream_t stream);
/* Surface normals for a scan that comes without them (a velodyne .bin, a live scan): the reference reads the normal from its
 * pc_npy_with_normal file (kitti.py:130) and computes it nowhere, so this contract is the project's own; parity with the third-party
 * estimator of the upstream preprocessing is unpinned.
 *   points (S, 3); idx (Q, ldi) int32 rows into points, dist (Q, ldi) their squared distances (NULL allowed when radius <= 0): row q is
 *       the neighbourhood of point q (Q <= S), as a self search cofi_knn_topk_grid / cofi_knn_topk returns it; the first k slots of a row
 *       are read (k <= 128, ldi >= k).  A slot is skipped when its index is >= S (the search's shadow padding) or, with radius > 0, its
 *       squared distance is > radius^2 ("at most k within radius"); m = slots kept.
 *   fp32: d = neighbour - query, C = sum d d^T / m - (sum d / m)(sum d / m)^T, normal = unit eigenvector of the smallest eigenvalue of C
 *       (cyclic Jacobi on the power-of-two scaled matrix + one first-order correction against the unrotated matrix).
 *   degenerate rows - m < 3, trace(C) == 0 (all neighbours coincide) or a non-finite result - get (0, 0, 1) and are counted into
 *       degenerate_count_dev[0] (optional; zeroed by the caller; one atomic per wave at most).
 *   sign: the component of largest magnitude positive (lowest axis on ties); then, with viewpoint3_dev (3 floats in device memory, NULL for
 *       none), flipped when n . (v - p) < 0.  A function of the input alone.
 *   out[q * out_point_stride + c * out_comp_stride], c = 0..2 (strides in floats): (N, 3) rows are (3, 1); rows 4..6 of a channel-major
 *       (7, N) scan are written in place with out = data7n + 4 * N, strides (1, N). */
int cofi_estimate_normals(const float *points, int S, const int32_t *idx, const float *dist, int Q, int k, int ldi, float radius,
                          const float *viewpoint3_dev, float *out, long long out_point_stride, long long out_comp_stride,
                          int32_t *degenerate_count_dev, cofi_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Registered clouds: the `images` = F = S * C images of a submission joined with its S = F / cameras clouds through the per-image poses
 * of the pose tail - z-buffered depth and point-id maps per image, in-picture / visible flags per (image, point), and per point the
 * colour of the camera that sees it most centrally.  The reference has offline numpy helpers only (data/kitti_helper.py:166-190
 * crop_pc_with_img, :142-163 projection_pc_img), without occlusion; the contract is this project's.  Operands are read in place:
 *   points  (S * N, 3), cloud s at rows s * N ...; image f looks at cloud f / cameras
 *   img     (F, Ci, H, W) float32
 *   pose    image f at pose + f * pose_stride floats (pose_stride >= 12): [R row-major | t], camera <- cloud, as cofi_pnp_ransac_batch /
 *           cofi_pnp_ransac_rig write their per-image poses
 *   result  optional (NULL: every image takes part): image f contributes nothing when result[f * result_stride] == 0
 *   K_dev   (F, 3, 3) float32 in DEVICE memory; fx, fy, cx, cy are each multiplied by k_scale (one fp32 product; the convention of
 *           camera_matrix_scaling, data/kitti.py:188-191: a half-resolution K serves the full image with k_scale = 2)
 * Projection (fp32, one device function for every pass, each operation a correctly rounded fma / division, no contraction): camera
 * coordinates by rows, fma(r2, Z, fma(r1, Y, fma(r0, X, t))); u = fma(fx, x / z, cx), v = fma(fy, y / z, cy); pixel = rintf (ties to even, as
 * np.round); in picture = z > z_near and 0 <= px <= W - 1 and 0 <= py <= H - 1, compared as floats so that a NaN is out.
 *   pass 1  every in-picture point: atomicMin of the key (float bits of z) << 32 | cloud-local point id on the (2 splat + 1)^2 pixels around
 *           its own, clipped to the image: the nearest point wins a pixel, the lowest id among equal depths, in any order of arrival
 *   pass 2  visible in a camera = in picture and z <= zmin * (1 + rel_tol) + abs_tol (one fma), zmin decoded from the key of its own pixel.
 *           Among the cameras that see a point the one with the smallest ((u - cx) / fx)^2 + ((v - cy) / fy)^2 gives the colour (lowest
 *           camera on ties): bilinear at (u, v), pixel centres at integer coordinates, the four taps clamped to the edge, weights
 *           (1-ax)(1-ay), ax(1-ay), (1-ax)ay, ax ay and the sum fma(w11, p11, fma(w10, p10, fma(w01, p01, w00 p00))).
 *   pass 3  keys -> maps
 * Outputs: depth (F, H, W) float32, 0 where empty; index (F, H, W) int32 cloud-local id, -1 where empty; flags (F, N) uint8, bit 0 in
 * picture, bit 1 visible; color (S, N, Ci) float32, 0 where unseen; camera (S, N) int32, -1 where unseen; stats (F, 4) int32 = {in
 * picture, visible, pixels hit, 0} (zeroed here; counted per workgroup, then one integer atomic each).  With splat > 0 a point can own a
 * neighbouring pixel while failing the gate at its own, so `index` may hold ids that are in picture but not visible; with splat 0 every id
 * in `index` is visible.  ws: cofi_fuse_workspace(F, H, W) = 8 bytes per pixel (0 for non-positive arguments or F * H * W beyond 31
 * bits), 8-byte aligned.  COFI_EINVAL: a NULL required pointer, non-positive sizes, cameras not dividing images, splat outside 0..3,
 * z_near or k_scale not positive, a negative tolerance, F * H * W beyond 31 bits; COFI_EWORKSPACE: ws too small; COFI_EUNSUPPORTED:
 * images > 65535.  Four launches on `stream` (the first clears the keys to the all-ones sentinel and the stats), no host synchronisation. */
size_t cofi_fuse_workspace(int images, int H, int W);
int cofi_fuse_cloud_image(const float *points, int N, int images, int cameras, const float *img, int Ci, int H, int W, const float *pose,
                          int pose_stride, const int32_t *result, int result_stride, const float *K_dev, float k_scale, float z_near,
                          int splat, float rel_tol, float abs_tol, void *ws, size_t ws_bytes, float *depth, int32_t *index, uint8_t *flags,
                          float *color, int32_t *camera, int32_t *stats, cofi_stream_t stream);

/* Batched device-to-device copy in one launch: descs_dev = n records {const void *src; void *dst; uint64 bytes} in device
 * memory (e.g. the per-frame inputs -> the static buffers of a captured forward graph); blocks_per_copy workgroups per record. */
int cofi_multi_copy(const void *descs_dev, int n, int blocks_per_copy, cofi_stream_t stream);

/* Row blocks repeated in place of a caller-side torch.repeat_interleave: src holds `frames` blocks of rows_per_frame rows (leading
 * dimension lds), dst `frames * times` such blocks (ldd), and
 *   dst[(s * times + c) * rows_per_frame + r, 0:cols] = src[s * rows_per_frame + r, 0:cols]   for s < frames, c < times.
 * Columns >= cols of dst are not touched: dst may be a column slice of a wider buffer (the coarse point tokens of one cloud copied
 * into the transformer's (rows, 2 * 128) point stream once per camera of a rig).  16-byte accesses when both pointers and both leading
 * dimensions are 16-byte aligned, with single floats for the cols % 4 rest; single floats throughout otherwise.  src and dst must not
 * overlap. */
int cofi_repeat_frames(const float *src, int lds, int rows_per_frame, int cols, int frames, int times, float *dst, int ldd,
                       cofi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* COFI_HIP_H */
