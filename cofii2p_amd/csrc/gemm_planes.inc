// bf16x3 contraction with BOTH operands pre-split into bf16 hi / lo planes (included by gemm.hip, inside its anonymous namespace).
//
//   C = A W^T with A = Ah + Al (M, K planes), W = Wh + Wl (N, K planes); products Al*Wh + Ah*Wl + Ah*Wh on v_mfma_f32_32x32x16_bf16,
//   fp32 accumulate - the same three MFMAs in the same order and the same ascending K order as gemm_bf16x3_kernel, so for equal
//   split-K chunks the two kernels produce identical bits.
//
// What differs is how the operands travel.  A split operand costs 4 bytes per element like fp32, but the bf16 matrix cores retire it
// 5.3x faster than the fp32 ones: the kernel is bound by the CU's fill path, not by the MFMA pipe, unless tiles move with no
// instruction overhead and no bubbles.  So:
//   * tiles go global -> LDS by LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16 B = 1 KiB per instruction, no VGPR staging, no ds_write,
//     no conversion VALU), NST LDS stages deep, with ONE barrier per K-tile:
//         wait vmcnt(tiles still allowed in flight) ; barrier ; issue tile t + NST - 1 into the stage freed by tile t - 1 ; MFMAs on tile t
//     The DMA is issued through inline asm: hipcc (ROCm 7.2) serialises an LDS-DMA it knows about against EVERY later ds_read
//     (s_waitcnt vmcnt(0) before the first fragment read of each K-tile, which empties the pipeline); the asm form keeps the queue
//     invisible to its scoreboard and the kernel counts vmcnt itself.  Ordering: a wave waits for ITS OWN DMA pieces of tile t, then
//     the barrier publishes all waves' pieces; the stage overwritten next was last read before that same barrier.
//   * the LDS image of a stage is [Ah | Al | Wh | Wl], plane rows of BK bf16 (BK * 2 bytes), 16-byte chunks XOR-swizzled so that the
//     ds_read_b128 fragment reads (lane = row, 16-lane groups {0-3,12-15,20-27} ...) hit 16 distinct 16-B slots of the 256-B bank
//     row: chunk' = chunk ^ ((row / rows-per-bank-row) & (chunks-per-row - 1)).  The DMA writes lane-linear, so the permutation is
//     applied to the per-lane SOURCE address (every instruction still covers whole 128-B / 64-B row segments).
//   * K tails and nothing else need zero fill: lanes whose chunk starts past the K range read a 16-byte zero page instead.
//     Rows past M / N are clamped to the last row (their results are never stored).
// The tail behind the K loop is the shared one (gemm.hip, mfma32_tile_tail: split-K partials, else 64-row slabs through rowwise_epilogue);
// the XCD tile order is that of the other kernels.

__device__ __attribute__((aligned(16))) unsigned g_zero_chunk[4];   // zero-initialised: the source of K-tail chunks

__device__ __forceinline__ void glds16_s(const void *sbase, unsigned voff, unsigned lds_addr) {   // uniform base + per-lane byte offset
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" : : "s"(lds_addr), "v"(voff), "s"(sbase) : "memory");
}
__device__ __forceinline__ void glds16_v(const void *vaddr, unsigned lds_addr) {                   // per-lane 64-bit address
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" : : "s"(lds_addr), "v"(vaddr) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N) : "memory");
}

template <int BM, int BN, int BK, int WM, int WN, int NST, int MINW>
__global__ __launch_bounds__(64 * WM * WN, MINW) void gemm_planes_kernel(GemmArgs g) {
    constexpr int NW = WM * WN, NT = 64 * NW;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static_assert(TM >= 1 && TN >= 1 && BM == WM * TM * 32 && BN == WN * TN * 32 && BM % 64 == 0, "wave grid must tile the block");
    constexpr int ROWB = BK * 2;          // bytes of a plane row in LDS
    constexpr int CPR = BK / 8;           // 16-byte chunks per row
    constexpr int RPB = 16 / CPR;         // rows per 256-byte bank row
    constexpr int RPI = 1024 / ROWB;      // rows per DMA instruction
    static_assert(BK == 32 || BK == 64 || BK == 128, "K-tile depth");
    constexpr int PLANE_A = BM * ROWB, PLANE_W = BN * ROWB, STAGE = 2 * (PLANE_A + PLANE_W);
    constexpr int NA = BM / RPI, NB = BN / RPI;            // 1 KiB pieces per plane
    static_assert(NA % NW == 0 && NB % NW == 0, "the pieces of a plane must divide over the waves");
    constexpr int JA = NA / NW, JB = NB / NW, LPT = 2 * (JA + JB);   // pieces per wave: per A plane, per W plane, per tile
    static_assert((NST - 2) * LPT <= 63 && NST >= 2 && NST <= 4, "vmcnt is a 6-bit counter");
    constexpr int TLD = BN + 4;
    constexpr int EPI = 64 * TLD * 4;
    constexpr int LDS_BYTES = NST * STAGE > EPI ? NST * STAGE : EPI;
    static_assert((NT / (BN / 4)) * BN * 2 * 4 <= EPI && 64 % (NT / (BN / 4)) == 0, "epilogue scratch / row passes");
    __shared__ __attribute__((aligned(1024))) unsigned char lds_raw[LDS_BYTES];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const BlockId bid = gemm_block_id(g);
    const int m0 = bid.y * BM, n0 = bid.x * BN;
    const int kbeg = bid.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int ntiles = (kend - kbeg + BK - 1) / BK;
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)lds_raw;

    // ---- DMA source map: lane p of piece q writes LDS chunk p of the piece = (row q * RPI + p / CPR, position p % CPR), which holds
    //      logical chunk (p % CPR) ^ swizzle(row)
    const int prow = lane / CPR, ppos = lane % CPR;
    unsigned voffA[JA], voffW[JB];
    int chA[JA], chW[JB];   // logical chunk of this lane (K-tail test)
#pragma unroll
    for (int j = 0; j < JA; ++j) {
        const int rl = (wave + NW * j) * RPI + prow;
        chA[j] = ppos ^ ((rl / RPB) & (CPR - 1));
        voffA[j] = ((unsigned)(min(m0 + rl, g.M - 1) - m0) * (unsigned)g.lda + 8u * chA[j]) * 2u;
    }
#pragma unroll
    for (int j = 0; j < JB; ++j) {
        const int rl = (wave + NW * j) * RPI + prow;
        chW[j] = ppos ^ ((rl / RPB) & (CPR - 1));
        voffW[j] = ((unsigned)(min(n0 + rl, g.N - 1) - n0) * (unsigned)g.ldw + 8u * chW[j]) * 2u;
    }
    const char *aH = reinterpret_cast<const char *>(reinterpret_cast<const uint16_t *>(g.A) + (size_t)m0 * g.lda + kbeg);
    const char *aL = aH + (size_t)g.a_lo_off * 2;
    const char *wH = reinterpret_cast<const char *>(reinterpret_cast<const uint16_t *>(g.W) + (size_t)n0 * g.ldw + kbeg);
    const char *wL = wH + (size_t)g.w_lo_off * 2;

    auto stage = [&](int t, int buf) {
        const unsigned lb = lds_base + buf * STAGE + wave * 1024;
        const size_t ko = (size_t)t * ROWB;
        if (kbeg + (t + 1) * BK <= kend) {   // full tile: uniform base + constant per-lane offsets, no vector arithmetic
#pragma unroll
            for (int j = 0; j < JA; ++j) {
                glds16_s(aH + ko, voffA[j], lb + NW * j * 1024);
                glds16_s(aL + ko, voffA[j], lb + PLANE_A + NW * j * 1024);
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                glds16_s(wH + ko, voffW[j], lb + 2 * PLANE_A + NW * j * 1024);
                glds16_s(wL + ko, voffW[j], lb + 2 * PLANE_A + PLANE_W + NW * j * 1024);
            }
        } else {                             // K tail: chunks past the range come from the zero page (K is a multiple of 8)
            const int kt = kbeg + t * BK;
#pragma unroll
            for (int j = 0; j < JA; ++j) {
                const bool in = kt + 8 * chA[j] < kend;
                glds16_v(in ? (const void *)(aH + ko + voffA[j]) : (const void *)g_zero_chunk, lb + NW * j * 1024);
                glds16_v(in ? (const void *)(aL + ko + voffA[j]) : (const void *)g_zero_chunk, lb + PLANE_A + NW * j * 1024);
            }
#pragma unroll
            for (int j = 0; j < JB; ++j) {
                const bool in = kt + 8 * chW[j] < kend;
                glds16_v(in ? (const void *)(wH + ko + voffW[j]) : (const void *)g_zero_chunk, lb + 2 * PLANE_A + NW * j * 1024);
                glds16_v(in ? (const void *)(wL + ko + voffW[j]) : (const void *)g_zero_chunk, lb + 2 * PLANE_A + PLANE_W + NW * j * 1024);
            }
        }
    };

    // one DMA piece of a FULL tile t (p = 0 .. LPT - 1, compile-time: A pieces [hi, lo] per row block first, then W) - the pipelined loop
    // spreads the pieces of a tile over the MFMA steps of the tile before it
    auto stage_piece = [&](int t, int buf, int p) {
        const bool isA = p < 2 * JA;
        const int q = isA ? p : p - 2 * JA, j = q >> 1, lo = q & 1;
        const unsigned lb = lds_base + buf * STAGE + wave * 1024 + NW * j * 1024 + (isA ? lo * PLANE_A : 2 * PLANE_A + lo * PLANE_W);
        glds16_s((isA ? (lo ? aL : aH) : (lo ? wL : wH)) + (size_t)t * ROWB, isA ? voffA[j] : voffW[j], lb);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // ---- fragment reads: lane (li, lh) owns k = 16 s + 8 lh .. + 7 of row li: chunk 2 s + lh, stored at chunk ^ swizzle(li)
    //      (the swizzle of a row depends on li only: the 32-row blocks start at multiples of 16 bank rows)
    const int li = lane & 31, lh = lane >> 5;
    const int swz = (li / RPB) & (CPR - 1);
    const unsigned arow = (unsigned)(wm * 32 * TM + li) * ROWB, wrow = 2u * PLANE_A + (unsigned)(wn * 32 * TN + li) * ROWB;
    union Frag { uint4 u; bf16x8 v; };
    constexpr int STEPS = BK / 16;
    // ---- main loop: NST - 1 tiles in flight
    {
        // Software-pipelined form: the fragments of step s + 1 are read while the MFMAs of step s run (two register sets, static
        // parity), the barrier that publishes tile t + 1 sits inside the LAST step of tile t - its first fragment reads are issued
        // before the MFMAs of that step - and the DMA pieces of tile t + NST - 1 are spread over the steps (a piece blocks the wave's
        // issue for 60-180 cycles: a few at a time next to MFMAs instead of LPT in a row).  A K tail (only ever the last tile) is
        // issued whole, at the first step.
        Frag fa[2][TM][2], fb[2][TN][2];
        auto rd = [&](int bf, int st, int par) {
            const unsigned char *sb = lds_raw + bf * STAGE;
            const unsigned co = (unsigned)((2 * st + lh) ^ swz) * 16u;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                fa[par][i][0].u = *reinterpret_cast<const uint4 *>(sb + arow + i * 32 * ROWB + co);
                fa[par][i][1].u = *reinterpret_cast<const uint4 *>(sb + PLANE_A + arow + i * 32 * ROWB + co);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                fb[par][j][0].u = *reinterpret_cast<const uint4 *>(sb + wrow + j * 32 * ROWB + co);
                fb[par][j][1].u = *reinterpret_cast<const uint4 *>(sb + PLANE_W + wrow + j * 32 * ROWB + co);
            }
        };
        auto mm = [&](int par) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[par][i][1].v, fb[par][j][0].v, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[par][i][0].v, fb[par][j][1].v, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[par][i][0].v, fb[par][j][0].v, acc[i][j], 0, 0, 0);
                }
        };
        auto wait_for = [&](int t) {   // tile t has landed; the tiles issued after it (at most NST - 2, all completely issued) stay in flight
            const int rem = min(NST - 2, ntiles - 1 - t);
            if (NST >= 4 && rem >= 2) wait_vmcnt<(NST >= 4 ? 2 * LPT : 0)>();
            else if (NST >= 3 && rem >= 1) wait_vmcnt<(NST >= 3 ? LPT : 0)>();
            else wait_vmcnt<0>();
        };
        const int nfull = (kend - kbeg) / BK;   // full tiles; tile nfull (if any) is the K tail
        // with two stages the tile being fetched is the one the last step waits for: its pieces go out during the earlier steps
        constexpr int PSTEPS = (NST == 2 && STEPS > 1) ? STEPS - 1 : STEPS;
#pragma unroll
        for (int s = 0; s < NST - 1; ++s)
            if (s < ntiles) stage(s, s);
        if (ntiles > 0) {
            wait_for(0);
            __syncthreads();
            rd(0, 0, 0);
        }
        int buf = 0, nbuf = NST - 1;
        for (int t = 0; t < ntiles; ++t) {
            const int tn = t + NST - 1;   // the tile issued during this one
            const int nxt = buf + 1 == NST ? 0 : buf + 1;
            if (tn >= nfull && tn < ntiles) stage(tn, nbuf);
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                if (tn < nfull) {
#pragma unroll
                    for (int p = 0; p < LPT; ++p)
                        if (p * PSTEPS / LPT == s) stage_piece(tn, nbuf, p);
                }
                if (s + 1 < STEPS) {
                    rd(buf, s + 1, (s + 1) & 1);
                } else if (t + 1 < ntiles) {
                    wait_for(t + 1);
                    __syncthreads();
                    rd(nxt, 0, 0);
                }
                mm(s & 1);
            }
            buf = nxt;
            nbuf = nbuf + 1 == NST ? 0 : nbuf + 1;
        }
    }

    // ---- split-K partials, or the epilogue in 64-row slabs through LDS
    mfma32_tile_tail<BM, BN, TM, TN, NT, false>(g, acc, reinterpret_cast<float *>(lds_raw), bid.z, m0, n0, wm, wn, li, lh, tid);
}
