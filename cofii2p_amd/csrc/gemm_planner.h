// gemm_planner.h - the host-side choice behind every contraction of gemm.hip: kernel family, tile, K split, f16x3 tile flags, workspace.
// Plain host C++ (no HIP types, no GemmArgs): a PlanRequest goes in, a status and a Plan come out.  The entries (gemm_entry, conv_entry,
// cofi_gemm_f32_layernorm), the queries (cofi_gemm_f16x3_eligible, cofi_conv2d_f16x3_eligible, cofi_gemm_f32_workspace) and the description
// hooks (cofi_tune_describe_gemm / _conv) all call plan_gemm / plan_conv; nothing else decides.  One translation unit includes this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/cofi_hip.h"
#include "../../include/cofi_hip_tune.h"

#ifndef COFI_CDIV_DEFINED
#define COFI_CDIV_DEFINED
static inline int cofi_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
#endif

namespace {

constexpr int PLAN_BK = 32;   // K-tile of the register-staged kernels (BK of gemm.hip)

// ---- the request: everything the choice depends on
struct PlanRequest {
    int M, N, K;            // the contraction; plan_conv derives them from the geometry below
    int act;                // what is left of the entry's `act` word once the flag bits are taken out (decode_flags)
    int arith;              // 0 fp32 MFMA, 1 bf16x3, 2 bf16x6
    int wsplit, asplit;     // COFI_GEMM_W_SPLIT / COFI_GEMM_A_SPLIT
    int l2n, fused_ln;      // a tile spans the whole row (N <= 128): COFI_GEMM_L2NORM / cofi_gemm_f32_layernorm
    int f16, wf16;          // COFI_GEMM_F16X3 / COFI_GEMM_W_F16PRE
    int pending_norm;       // 0 none, 1 the A operand carries a pending normalisation (statistics partials), 2 ... finalised (scale_shift)
    int frames;             // stacked frames; M / frames rows each
    size_t ws_bytes;        // workspace on offer (0: none)
    // What only the entry can check, reported at the place the entries have always reported it: leading dimensions and statistics width
    // against the flags (false: COFI_EINVAL), the pending norm's descriptor (make_norm_src's status).  A description assumes legal operands.
    bool operands_ok;
    int norm_status;
    // convolution (ks != 0): NHWC input of `frames` maps H x W x Cin in rows of ldx floats
    int H, W, Cin, Cout, ks, stride, pad, ldx;
};

// the flag bits of an entry's `act` word
inline PlanRequest decode_flags(int act) {
    PlanRequest r{};
    r.arith = (act & COFI_GEMM_BF16X6) ? 2 : ((act & COFI_GEMM_BF16X3) ? 1 : 0);
    r.wsplit = (act & COFI_GEMM_W_SPLIT) ? 1 : 0;
    r.asplit = (act & COFI_GEMM_A_SPLIT) ? 1 : 0;
    r.l2n = (act & COFI_GEMM_L2NORM) ? 1 : 0;
    r.f16 = (act & COFI_GEMM_F16X3) ? 1 : 0;
    r.wf16 = (act & COFI_GEMM_W_F16PRE) ? 1 : 0;
    r.act = act & ~(COFI_GEMM_BF16X3 | COFI_GEMM_BF16X6 | COFI_GEMM_W_SPLIT | COFI_GEMM_A_SPLIT | COFI_GEMM_L2NORM | COFI_GEMM_F16X3 | COFI_GEMM_W_F16PRE);
    r.frames = 1;
    r.operands_ok = true;
    return r;
}

// ---- the plan
struct Plan {
    int family;   // COFI_PLAN_* (include/cofi_hip_tune.h): the kernel launch() takes
    int bm, bn, ksplit, kchunk;
    int pcfg;   // >= 0: gemm_planes_kernel configuration (kPlanesCfg) - both operands are bf16 planes; -1: the register-staged kernels
    int big;    // 1: gemm_x6_big_kernel (bf16x6, 256 x 128 tile, one workgroup per CU) or, with tile flags, gemm_f16_big_kernel
    size_t partial_bytes;   // split-K partials at the start of the workspace
    long long flag_off;     // byte offset of the f16x3 kernels' tile flags (behind the partials); -1: none, the launch is not an f16x3 one
    size_t ws_bytes;        // partials, then flags: what this plan uses of the workspace
};

// Configurations of gemm_planes_kernel: tile, K-tile depth, wave grid, LDS stages, workgroups per CU the register budget allows.
struct PlanesCfg { int bm, bn, bk, wm, wn, nst, minw; };
#define COFI_PLANES_CFGS(X)          \
    X(0, 128, 128, 64, 4, 2, 2, 2)   \
    X(1, 64, 64, 64, 2, 2, 2, 2)     \
    X(2, 256, 128, 32, 4, 2, 3, 2)   \
    X(3, 256, 256, 32, 4, 2, 2, 2)   \
    X(4, 128, 32, 64, 4, 1, 2, 2)    \
    X(5, 128, 64, 64, 4, 2, 2, 2)    \
    X(6, 64, 64, 32, 2, 2, 4, 2)     \
    X(7, 128, 128, 32, 4, 2, 4, 2)   \
    X(8, 64, 128, 64, 2, 2, 2, 1)
static const PlanesCfg kPlanesCfg[] = {
#define X(id, bm, bn, bk, wm, wn, nst, minw) {bm, bn, bk, wm, wn, nst, minw},
    COFI_PLANES_CFGS(X)
#undef X
};
constexpr int kNumPlanesCfg = sizeof(kPlanesCfg) / sizeof(kPlanesCfg[0]);

// Tuned plans for the shapes of the KITTI / nuScenes-shaped forward (tools/tune_gemm.py on MI355X, bf16x3 kernel):
// {M, N, K, bm, bn, ksplit}.  Anything not listed falls through to the heuristic below.
struct TunedPlan { int M, N, K, bm, bn, ks; };
#include "gemm_plans.inc"
// ... and for the bf16x6 kernel (twice the MFMAs and 1.5x the LDS traffic per K-tile move the best split): tools/tune_gemm.py --gemm bf16x6
#include "gemm_plans_x6.inc"

// Tuning / test hooks (include/cofi_hip_tune.h): plan overrides of the CALLING THREAD only - plans are chosen on the thread that enqueues a
// launch, so a tool or a test that forces a plan cannot change the launches of any other thread; the product path never sets them.
thread_local int g_force_bm = 0, g_force_bn = 0, g_force_ks = 0;

// k-chunks in multiples of 128: the bf16x3 kernel steps K by 128
inline void split_k(Plan &p, int K, int ks) {
    const int ktiles = cofi_cdiv(K, PLAN_BK);
    int tiles_per = cofi_cdiv(ktiles, ks < 1 ? 1 : ks);
    tiles_per = (tiles_per + 3) & ~3;
    p.kchunk = tiles_per * PLAN_BK;
    p.ksplit = cofi_cdiv(K, p.kchunk);
}

inline Plan finish_plan(int K, int bm, int bn, int ks) {
    Plan p{};
    p.pcfg = -1;
    p.bm = bm; p.bn = bn;
    split_k(p, K, ks);
    return p;
}

// Heuristic: largest tile that still gives >= ~1 workgroup per CU, then split K until the chip
// (256 CUs) is covered about twice, keeping >= 2 k-tiles (64 values) per split.
inline Plan make_plan_unwidened(int M, int N, int K, int arith) {
    if (g_force_bm)
        return finish_plan(K, g_force_bm, (g_force_bm == 128 && g_force_bn == 64 && arith != 2) ? 128 : g_force_bn, g_force_ks);   // 128 x 64: bf16x6 only
    static const bool x6_table = !(getenv("COFI_GEMM_X6_PLANS") && atoi(getenv("COFI_GEMM_X6_PLANS")) == 0);   // A/B switch (tools)
    if (arith == 2 && x6_table)
        for (const TunedPlan &t : kTunedPlansX6)
            if (t.M == M && t.N == N && t.K == K) return finish_plan(K, t.bm, t.bn, t.ks);
    for (const TunedPlan &t : kTunedPlans)
        if (t.M == M && t.N == N && t.K == K) return finish_plan(K, t.bm, t.bn, t.ks);
    Plan p{};
    p.pcfg = -1;
    auto blocks = [&](int bm, int bn) { return (long)cofi_cdiv(M, bm) * cofi_cdiv(N, bn); };
    if (N > 64 && M > 64 && blocks(128, 128) >= 200) {
        p.bm = 128; p.bn = 128;
    } else if (N > 64 && blocks(64, 128) >= 200) {
        p.bm = 64; p.bn = 128;
    } else if (N > 32) {
        p.bm = 64; p.bn = 64;
        if (N > 64 && blocks(64, 128) * 2 >= blocks(64, 64) && blocks(64, 64) > 1024) { p.bn = 128; }
    } else {
        p.bm = 64; p.bn = 64;
    }
    long nb = blocks(p.bm, p.bn);
    int ktiles = cofi_cdiv(K, PLAN_BK);
    int ks = 1;
    // Split K only when the serial k-loop is long: a split costs a second kernel (the reduction epilogue,
    // ~5 us of launch + latency), which a loop of <= 16 k-tiles (K <= 512) cannot win back.
    if (nb < 384 && ktiles > 16) {
        ks = (int)((512 + nb - 1) / nb);
        int maxks = ktiles / 8;  // >= 256 k-values per split
        if (maxks < 1) maxks = 1;
        if (ks > maxks) ks = maxks;
        if (ks > 32) ks = 32;
    }
    split_k(p, K, ks);
    return p;
}

inline Plan make_plan_base(int M, int N, int K, bool fused_ln, int arith) {
    Plan p = make_plan_unwidened(M, N, K, arith);
    if (fused_ln && p.ksplit == 1 && p.bn < N) {  // un-split: one tile must span the whole row (N <= 128)
        p.bm = 64;
        p.bn = 128;
    }
    return p;
}

// bf16x6, <= 64 output columns over many rows (stack-mode batches of >= 4 frames): a 128 x 64 tile (waves of 64 x 32) splits a W tile once
// per 128 rows instead of once per 64 and reads 3/4 of the fragment bytes per MFMA.  Measured on the batch-16 shapes (tools/tall_tile_probe.py,
// outputs bit-equal to the 64 x 64 tile's): -12 ... -31 % per launch from 640 tiles up (M >= 81920), +-3 % at 320 tiles, +35 % at 160 - hence
// the threshold.  COFI_GEMM_TALL_TILE=0 switches it off (A/B), any other value is the threshold in tiles.
inline Plan make_plan(int M, int N, int K, bool fused_ln, int arith) {   // arith: PlanRequest::arith (2 = bf16x6: its own table first)
    Plan p = make_plan_base(M, N, K, fused_ln, arith);
    static const long tall = getenv("COFI_GEMM_TALL_TILE") ? atol(getenv("COFI_GEMM_TALL_TILE")) : 512;
    if (arith == 2 && !g_force_bm && tall > 0 && p.pcfg < 0 && p.bm == 64 && p.bn == 64 && p.ksplit == 1 && N <= 64 &&
        (long)cofi_cdiv(M, 128) * cofi_cdiv(N, 64) >= tall)
        p.bm = 128;
    return p;
}

// ---- gemm_x6_big_kernel (256 x 128 tiles, ONE workgroup per CU): which shapes take it, and with which K split.
// One workgroup per CU means whole rounds of 256 workgroups: a grid of 320 tiles takes two rounds like one of 512.  The split is chosen
// to minimise  rounds x (k-tiles per workgroup + fixed cost)  plus the partial-sum traffic a split adds (ks x M x N x 4 bytes written
// and read again), in units of one K-tile of the main loop (~1.5 us).
// tuning hook (tools only): g_force_big = 1 forces the kernel on every eligible launch (split g_force_big_ks, 0 = chosen here), -1 disables it
thread_local int g_force_big = 0, g_force_big_ks = 0, g_big_dbg = 0;
thread_local int g_force_direct = 0;   // tools / tests: 1 = the direct 3 x 3 kernel on every eligible convolution (no tile-count threshold), 2 = ... with 4-row tiles, -1 = never, 0 = default
struct TunedBig { int M, N, K, ks; };   // ks = 0: keep the small-tile kernel for this shape
#include "gemm_plans_big.inc"

inline bool big_plan(int M, int N, int K, Plan &p, bool f16 = false) {   // f16: the launch will run gemm_f16_big_kernel (COFI_GEMM_F16X3)
    static const int mode = getenv("COFI_GEMM_BIG") ? atoi(getenv("COFI_GEMM_BIG")) : 1;   // A/B switch: 0 = never
    if (g_force_big < 0 || (mode == 0 && g_force_big == 0) || g_force_bm) return false;
    // N <= 64: the 256 x 64 instantiation of the kernel (four waves of 64 x 64) exists in the template and is bit-equal, but LOSES to the
    // 128 x 64 small tiles (round 5 probe, profiles/r05/big_gemm_probe_n64.txt: 327680 x 64 x 576 222 vs 209 us, 81920 x 64 x 576 80 vs 64 us -
    // the split of the A operand is 4.6 VALU instructions per MFMA there, and one workgroup per CU has nobody to overlap them with): not built.
    if ((K % 32) || N < 128 || M < 256) return false;
    const int bn = 128;
    const long tiles = (long)cofi_cdiv(M, 256) * cofi_cdiv(N, bn);
    const int ktiles = K / 32;
    int ks = 0;
    if (g_force_big > 0 && g_force_big_ks > 0) ks = g_force_big_ks;
    if (!ks && g_force_big == 0) {
        bool listed = false;
        static const int f16_table = getenv("COFI_GEMM_F16_TABLE") ? atoi(getenv("COFI_GEMM_F16_TABLE")) : 1;   // A/B switch: 0 = the six-product kernel's table and thresholds
        if (!f16_table) f16 = false;
        if (f16)
            for (const TunedBig &t : kTunedBigF16)
                if (t.M == M && t.N == N && t.K == K) { ks = t.ks; listed = true; break; }
        if (!listed)
            for (const TunedBig &t : kTunedBig)
                if (t.M == M && t.N == N && t.K == K) { ks = t.ks; listed = true; break; }
        if (listed && ks == 0) return false;
        if (!listed && (tiles < 160 || K < (f16 ? 256 : 512))) return false;   // short loops / small grids: two or three small workgroups per CU overlap their prologues and epilogues
        if (!listed && K < 512) ks = 1;
    }
    // The f16x3 kernel never splits K from this many 128 x 128 tiles up (COFI_GEMM_F16_KS1_TILES, 0 = off: the table's / cost model's splits
    // everywhere).  A split pays for a launch that runs ALONE on the chip - it fills idle CUs - and that is how the table was measured; beside
    // the other submissions of a pipeline its partial sums are only extra traffic and a fold launch.  Same box, frames/s with the splits /
    // capped at 80 / never split: batch 16 827 / 837 / 842 (another box 825 at 80, 824 never), batch 1 511 / 515 / 506, stress (one frame,
    // nothing else in flight) 59.5 / - / 58.4 with 59.4 at 160: small grids still need their splits (profiles/r06/ab_ks1*.txt).
    static const long ks1_tiles = getenv("COFI_GEMM_F16_KS1_TILES") ? atol(getenv("COFI_GEMM_F16_KS1_TILES")) : 80;
    if (f16 && ks1_tiles > 0 && g_force_big == 0 && (long)cofi_cdiv(M, 128) * cofi_cdiv(N, 128) >= ks1_tiles) ks = 1;
    if (!ks) {
        double best = 1e30;
        for (int c = 1; c <= 8; ++c) {
            const int chunk = cofi_cdiv(cofi_cdiv(ktiles, c), 4) * 4;   // k-chunks in multiples of 128, as the other kernels
            const int eff = cofi_cdiv(ktiles, chunk);
            if (eff != c || chunk < 8) continue;
            // f16x3 (pre-split W): 128 x 128 tiles, two workgroups per CU; else one 256 x 128 workgroup per CU
            const double rounds = f16 ? (double)cofi_cdiv((long)cofi_cdiv(M, 128) * cofi_cdiv(N, bn) * c, 512) : (double)cofi_cdiv(tiles * c, 256);
            const double partial = c > 1 ? 2.0 * c * (double)M * N * 4.0 / 4.0e12 / 1.5e-6 : 0.0;   // in K-tile units
            const double cost = rounds * (chunk + 6.0) + partial + (c > 1 ? 4.0 : 0.0);
            if (cost < best) { best = cost; ks = c; }
        }
        if (!ks) return false;
    }
    p.pcfg = -1;
    p.big = 1;
    p.bm = 256; p.bn = bn;
    const int chunk = cofi_cdiv(cofi_cdiv(ktiles, ks), 4) * 4;
    p.kchunk = chunk * 32;
    p.ksplit = cofi_cdiv(K, p.kchunk);
    return true;
}

// f16x3 kernel with pre-split W: 128 x 128 tiles, two workgroups per CU, instead of one 256 x 128 workgroup (gemm_f16_big.inc).
// Measured on the large contractions of a batch-16 forward (tools/f16_probe.py, profiles/r06/f16_probe_bm256.txt / _bm128.txt, same K splits):
// 8.81 -> 8.28 ms per submission, 27 of 29 shapes faster.  COFI_GEMM_F16_BM256=1 / cofi_tune_big_debug bit 512 (A/B): the 256-row form.
inline bool f16_two_per_cu() {
    static const int bm256 = getenv("COFI_GEMM_F16_BM256") ? atoi(getenv("COFI_GEMM_F16_BM256")) : 0;
    return !bm256 && (g_big_dbg & 512) == 0;
}

// bytes of the f16x3 kernels' tile-flag table: one word per workgroup of a 256 x 128 launch with `ks` K-slices
inline size_t f16_flag_bytes(int M, int N, int ks, int bm = 128) { return (size_t)cofi_cdiv(M, bm) * cofi_cdiv(N, 128) * ks * sizeof(unsigned); }   // (sized for the 128-row tiles: covers both forms)

// ---- plans of gemm_planes_kernel (both operands pre-split): {M, N, K, configuration, split-K}, tuned on MI355X by
// tools/tune_gemm.py --planes; anything not listed falls through to the heuristic.
struct TunedPlanes { int M, N, K, cfg, ks; };
#include "gemm_planes_plans.inc"

// tuning hook (tools/tune_gemm.py only): cfg >= 0 forces that configuration and split, -2 sends pre-split operands to the
// register-staged kernel instead (the A/B partner of the bit-identity test), -1 restores table + heuristic
thread_local int g_force_pcfg = -1, g_force_pks = 0;

inline Plan finish_planes_plan(int K, int cfg, int ks) {
    Plan p{};
    p.pcfg = cfg;
    p.bm = kPlanesCfg[cfg].bm;
    p.bn = kPlanesCfg[cfg].bn;
    const int ktiles = cofi_cdiv(K, 128);   // K chunks in multiples of 128, as finish_plan: equal splits give equal bits in both kernels
    if (ks < 1) ks = 1;
    p.kchunk = cofi_cdiv(ktiles, ks) * 128;
    p.ksplit = cofi_cdiv(K, p.kchunk);
    return p;
}

inline Plan make_planes_plan(int M, int N, int K) {
    if (g_force_pcfg >= 0 && g_force_pcfg < kNumPlanesCfg) return finish_planes_plan(K, g_force_pcfg, g_force_pks);
    for (const TunedPlanes &t : kTunedPlanes)
        if (t.M == M && t.N == N && t.K == K && t.cfg >= 0 && t.cfg < kNumPlanesCfg) return finish_planes_plan(K, t.cfg, t.ks);
    auto nblk = [&](int c) { return (long)cofi_cdiv(M, kPlanesCfg[c].bm) * cofi_cdiv(N, kPlanesCfg[c].bn); };
    const int max_ks = K >= 1024 ? K / 512 : 1;   // >= 512 K values (4 x 128) per split
    int cfg;
    if (N <= 32) cfg = 4;                          // 128 x 32
    else if (N <= 64) cfg = nblk(5) >= 400 ? 5 : 1;
    else if (nblk(3) * max_ks >= 400 && N % 256 == 0 && M >= 8192) cfg = 3;   // 256 x 256: the L2 -> LDS traffic of a tile halves again
    else if (nblk(2) >= 512) cfg = 2;              // 256 x 128
    else if (nblk(0) * max_ks >= 200) cfg = 0;     // 128 x 128
    else cfg = 1;                                  // 64 x 64
    const long nb = nblk(cfg);
    int ks = 1;
    if (nb < 200) {
        ks = (int)((256 + nb - 1) / nb);
        if (ks > max_ks) ks = max_ks;
        if (ks > 32) ks = 32;
    }
    return finish_planes_plan(K, cfg, ks);
}

// ---- the one ladder.  Statuses in the order the entries have always reported them.

// illegal / unsupported flag combinations
inline int check_flags(const PlanRequest &r) {
    const bool conv = r.ks != 0;
    if (r.wf16 && (!r.f16 || r.wsplit)) return COFI_EINVAL;
    const bool bad = (!r.fused_ln && (r.act < 0 || r.act > 3)) || (r.wsplit && r.arith == 0) || r.frames <= 0 || (conv && r.asplit);
    if (conv && bad) return COFI_EINVAL;   // (a convolution reports these before the L2-norm limit, a dense contraction after it)
    if (r.l2n && (r.N > 128 || r.asplit)) return COFI_EUNSUPPORTED;
    if (bad || !r.operands_ok || (r.fused_ln && r.N > 128)) return COFI_EINVAL;
    if (r.asplit && (r.arith != 1 || !r.wsplit || r.pending_norm || (r.K & 7))) return COFI_EINVAL;
    return 0;
}

// The contraction r.M x r.N x r.K.  big_ok: the operand geometry admits the 256 x 128 kernels (a dense A always does).
inline int plan_contraction(const PlanRequest &r, bool big_ok, Plan &p) {
    const int M = r.M, N = r.N, K = r.K;
    const int frame_rows = M / r.frames;
    const bool norm_frames = r.pending_norm && r.frames > 1;   // a normalising tile stays inside one frame
    p = (r.asplit && g_force_pcfg != -2) ? make_planes_plan(M, N, K) : make_plan(M, N, K, r.l2n || r.fused_ln, r.arith);
    if (big_ok && r.arith == 2 && !r.wsplit && !r.asplit && !r.l2n && !r.fused_ln && !(norm_frames && frame_rows % 256))
        big_plan(M, N, K, p, r.f16 != 0);   // the 256 x 128 kernel for the large shapes
    if (norm_frames && p.pcfg < 0 && p.bm == 128 && p.bn == 64 && frame_rows % 128) p.bm = 64;
    p.partial_bytes = p.ksplit > 1 ? (size_t)p.ksplit * M * N * sizeof(float) : 0;
    if (p.partial_bytes > r.ws_bytes) return COFI_EWORKSPACE;
    if (r.f16 && p.big && r.wf16 && f16_two_per_cu()) p.bm = 128;
    // the tile flags live behind this plan's split-K partials; a workspace without room for them: the six-product kernel
    p.flag_off = -1;
    p.ws_bytes = p.partial_bytes;
    if (r.f16 && p.big && r.ws_bytes >= p.partial_bytes + f16_flag_bytes(M, N, p.ksplit)) {
        p.flag_off = (long long)p.partial_bytes;
        p.ws_bytes += f16_flag_bytes(M, N, p.ksplit);
    }
    // a pre-split W is readable by gemm_f16_big_kernel only: the caller asks cofi_gemm_f16x3_eligible first
    if (r.wf16 && p.flag_off < 0) return COFI_EUNSUPPORTED;
    if (r.pending_norm) {   // runs on the bf16x3 kernels with pre-split weights and on the bf16x6 kernels
        if (!(r.arith == 1 && r.wsplit) && r.arith != 2) return COFI_EUNSUPPORTED;   // 3-term kernel: pre-split weights; 6-term kernel: fp32 or pre-split weights
        if (r.norm_status) return r.norm_status;
        if (r.frames > 1 && (M % r.frames || frame_rows % p.bm)) return COFI_EUNSUPPORTED;   // a tile of GEMM rows must lie inside one frame
    }
    if (p.pcfg >= 0) p.family = COFI_PLAN_PLANES;
    else if (p.big && p.flag_off < 0) p.family = COFI_PLAN_BIG_X6;
    else if (p.big && r.wf16) p.family = p.bm == 128 ? COFI_PLAN_BIG_F16_128 : COFI_PLAN_BIG_F16;   // pre-split W: eight-wave geometry only
    else if (p.big) p.family = (g_big_dbg & 256) ? COFI_PLAN_BIG_F16_W4 : COFI_PLAN_BIG_F16;
    else p.family = r.arith == 2 ? COFI_PLAN_BF16X6 : (r.arith ? COFI_PLAN_BF16X3 : COFI_PLAN_F32);
    return 0;
}

inline bool plan_is_f16x3(const Plan &p) { return p.family == COFI_PLAN_BIG_F16 || p.family == COFI_PLAN_BIG_F16_W4 || p.family == COFI_PLAN_BIG_F16_128; }
inline bool plan_is_direct(const Plan &p) { return p.family == COFI_PLAN_DIRECT_2 || p.family == COFI_PLAN_DIRECT_4; }

inline int plan_gemm(const PlanRequest &r, Plan &p) {
    if (r.M < 0 || r.N <= 0 || r.K <= 0) return COFI_EINVAL;
    if (int rc = check_flags(r)) return rc;
    return plan_contraction(r, true, p);
}

inline int conv_out_size(int in, const PlanRequest &r) { return (in + 2 * r.pad - r.ks) / r.stride + 1; }

// the contraction of a convolution, Ho * Wo * frames x Cout x ks * ks * Cin, into r.M, r.N, r.K; false: no such convolution
inline bool conv_contraction(PlanRequest &r) {
    if (r.H <= 0 || r.W <= 0 || r.Cin <= 0 || r.Cout <= 0 || (r.ks != 1 && r.ks != 3) || r.stride <= 0 || r.pad < 0 || r.frames <= 0) return false;
    r.M = conv_out_size(r.H, r) * conv_out_size(r.W, r) * r.frames;
    r.N = r.Cout;
    r.K = r.ks * r.ks * r.Cin;
    return true;
}

// A convolution: its own preconditions, then the contraction's ladder.
inline int plan_conv(PlanRequest &r, Plan &p) {
    if (!conv_contraction(r)) return COFI_EINVAL;
    if (int rc = check_flags(r)) return rc;
    const bool in32 = (size_t)r.frames * r.H * r.W * r.ldx * sizeof(float) < 0xffffffffull;   // 32-bit byte offsets into the input
    // narrow 3 x 3 convolutions of a stack-mode batch: the direct kernel (conv_direct.inc: input halo split once, 9 taps read it shifted)
    static const int direct_env = getenv("COFI_CONV_DIRECT") ? atoi(getenv("COFI_CONV_DIRECT")) : 1;   // A/B switch: 0 = never
    const int mode = g_force_direct ? g_force_direct : (direct_env ? 0 : -1);
    const long tiles4 = (long)r.frames * (r.H / 4) * (r.W / 64);
    const int th = (tiles4 >= 768 || g_force_direct == 2) ? 4 : 2;   // 4-row tiles once they fill the chip's workgroup slots (2 per CU) one and a half times
    const long tiles = (long)r.frames * (r.H / th) * (r.W / 64);
    const bool ok = r.arith == 2 && !r.wsplit && !r.l2n && r.ks == 3 && r.stride == 1 && r.pad == 1 && r.Cout == 64 && (r.Cin % 16) == 0 && r.Cin <= 512 &&
                    (r.W % 64) == 0 && (r.H % 4) == 0 && r.pending_norm != 1 && in32 && (size_t)r.Cout * r.K * sizeof(float) < 0xffffffffull;
    if (ok && !r.wf16 && mode >= 0 && (mode > 0 || tiles >= 256) && !g_force_bm) {
        p = Plan{};
        p.family = th == 4 ? COFI_PLAN_DIRECT_4 : COFI_PLAN_DIRECT_2;
        p.bm = 64; p.bn = 64; p.ksplit = 1; p.pcfg = -1; p.flag_off = -1;
        return r.pending_norm ? r.norm_status : 0;
    }
    // the 256 x 128 kernel: 3 x 3 / stride 1 / pad <= 1 convolutions whose K-tiles of 32 lie inside one tap
    return plan_contraction(r, r.ks == 3 && r.stride == 1 && r.pad <= 1 && (r.Cin % 32) == 0 && in32, p);
}

}  // namespace
