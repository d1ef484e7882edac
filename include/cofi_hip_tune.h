/*
 * cofi_hip_tune.h — tuning / test hooks of libcofi_hip.so.  NOT part of the drop-in ABI (include/cofi_hip.h): nothing in
 * cofii2p_amd/ or model/ calls these; tools/ (plan sweeps, A/B probes) and tests/ (bit-equality of one contraction under
 * two tilings) do.
 *
 * Every hook sets an override of the CALLING THREAD only (thread_local in csrc/gemm_planner.h): plans are chosen on the thread
 * that enqueues a launch, so a tool or test forcing a plan cannot change what any other thread - a serving thread, a
 * loader thread - launches.  Overrides stay until reset by the value documented as "default".  The results of a forced
 * plan are those of the same contraction under another tiling / K split (the tests compare them bit for bit where the
 * summation order is equal); no hook changes numerics beyond that.
 */
#ifndef COFI_HIP_TUNE_H
#define COFI_HIP_TUNE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Register-staged kernels (cofi_gemm_f32* / cofi_conv2d_nhwc*): force the tile (bm, bn in {64, 128}; 128 x 64 exists for the
 * bf16x6 arithmetic only) and the K split of every following plan; ksplit 0 = as the plan would choose.  (0, 0, 0) = default
 * (plan tables + heuristic).  Also keeps the 256 x 128 and the direct 3 x 3 kernels off while a tile is forced. */
int cofi_tune_force_plan(int bm, int bn, int ksplit);

/* Pre-split-operand kernel (COFI_GEMM_A_SPLIT): cfg >= 0 = that row of the configuration table with `ksplit`; -2 = send
 * pre-split operands to the register-staged kernel instead; -1 = default. */
int cofi_tune_force_planes(int cfg, int ksplit);

/* 256 x 128 one-workgroup-per-CU kernels (bf16x6 and f16x3): mode 1 = on every eligible launch (ksplit 0 = the cost model's
 * split), -1 = never, 0 = default (table + cost model). */
int cofi_tune_force_big(int mode, int ksplit);

/* Direct 3 x 3 convolution (64 output channels): 1 = on every eligible convolution regardless of the tile count, 2 = ... with
 * 4-row tiles, -1 = never, 0 = default. */
int cofi_tune_force_conv_direct(int mode);

/* Bit 64: the generic row-wise epilogue instead of the straight-line one (identical bits, slower: the A/B of DESIGN 14.3).
 * Bit 256: the f16x3 kernel in its four-wave geometry (one wave per SIMD) instead of the eight-wave one (identical bits).
 * Bit 512: the f16x3 kernel with pre-split weights in its 256-row one-workgroup-per-CU form instead of 128 x 128 tiles, two per CU.
 * Other bits are unused.  0 = default. */
int cofi_tune_big_debug(int flags);

/* Diagnostic of the f16x3 kernel (COFI_GEMM_F16X3): K-tiles re-split because they left the fp16 window of their panel's running scale,
 * summed over all launches since the last reset (a device-side counter; the call synchronises the device).  reset != 0: zero it after
 * reading.  -1 on error. */
long cofi_tune_f16x3_resplit_events(int reset);

/* Host-side census: contractions the calling thread enqueued (or captured) on the f16x3 kernel since the last reset -> their count;
 * *flops (optional) = the sum of their 2 M N K.  bench.py prices a launch list that mixes the six-product and the three-product kernel
 * against the mix of their two matrix roofs with it.  reset != 0: zero both after reading. */
long cofi_tune_f16x3_launch_flops(int reset, double *flops);

/* ---- Plan descriptions.  Every contraction is planned on the host by csrc/gemm_planner.h: a request (shape, decoded COFI_GEMM_* flags,
 * pending norm, frames, workspace on offer; for a convolution its geometry) goes in, a status and a plan come out.  The two hooks below run
 * that planner - under the calling thread's overrides - and launch nothing: they need no GPU.  tests/test_gemm_plans_cpu.py holds every plan
 * of a fixed request set against tests/golden/gemm_plans.npz with them. */
enum {
    COFI_PLAN_F32 = 0,         /* register-staged kernel, exact fp32 MFMA */
    COFI_PLAN_BF16X3 = 1,      /* register-staged kernel, three bf16 products */
    COFI_PLAN_BF16X6 = 2,      /* register-staged kernel, six bf16 products */
    COFI_PLAN_PLANES = 3,      /* both operands pre-split (COFI_GEMM_A_SPLIT): gemm_planes_kernel, configuration `pcfg` */
    COFI_PLAN_BIG_X6 = 4,      /* 256 x 128, one workgroup per CU, six bf16 products */
    COFI_PLAN_BIG_F16 = 5,     /* f16x3 kernel, 256 x 128, eight waves (fp32 or pre-split W) */
    COFI_PLAN_BIG_F16_W4 = 6,  /* f16x3 kernel, 256 x 128, four waves (cofi_tune_big_debug bit 256) */
    COFI_PLAN_BIG_F16_128 = 7, /* f16x3 kernel, pre-split W, 128 x 128 tiles, two workgroups per CU */
    COFI_PLAN_DIRECT_2 = 8,    /* direct 3 x 3 convolution, 2-row tiles */
    COFI_PLAN_DIRECT_4 = 9     /* direct 3 x 3 convolution, 4-row tiles */
};

typedef struct cofi_plan_desc {
    int status;                /* 0 or the COFI_E* code the entry returns from its planning stage; every other field is 0 unless status == 0 */
    int family;                /* COFI_PLAN_* */
    int bm, bn, ksplit, kchunk;
    int pcfg;                  /* COFI_PLAN_PLANES: row of the configuration table; -1 otherwise */
    long long partial_bytes;   /* split-K partials at the start of the workspace (0: no split) */
    long long flag_offset;     /* f16x3 families: byte offset of the tile-flag table in the workspace; -1: none */
    long long ws_bytes;        /* workspace bytes this plan uses: partials, then the flag table */
} cofi_plan_desc_t;

/* The plan of cofi_gemm_f32 / _colstats / _fused / _fused_res (fused_ln = 0) or of cofi_gemm_f32_layernorm (fused_ln = 1: `act` is its
 * `relu` word, N <= 128) for operands whose pointers and leading dimensions are legal.  act: the entry's `act` word (activation 0 ... 3 |
 * COFI_GEMM_* flags); pending_norm: 0 none, 1 the A operand carries a pending normalisation; ws_bytes: the workspace on offer (0: none).
 * Returns out->status. */
int cofi_tune_describe_gemm(int M, int N, int K, int act, int fused_ln, int pending_norm, int frames, size_t ws_bytes, cofi_plan_desc_t *out);

/* The plan of cofi_conv2d_nhwc / _fused.  pending_norm: 0 none, 1 statistics partials, 2 finalised (scale_shift set: the form the direct
 * 3 x 3 kernel reads).  M, N, K of the contraction are Ho * Wo * frames, Cout, ks * ks * Cin.  Returns out->status. */
int cofi_tune_describe_conv(int H, int W, int Cin, int Cout, int ks, int stride, int pad, int ldx, int act, int pending_norm, int frames,
                            size_t ws_bytes, cofi_plan_desc_t *out);

#ifdef __cplusplus
}
#endif
#endif
