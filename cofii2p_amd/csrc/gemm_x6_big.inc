// bf16x6 contraction for the LARGE shapes: one workgroup per CU, 256 x 128 output tile, all 512 registers of a wave (included by gemm.hip,
// inside its anonymous namespace).
//
// Same arithmetic as gemm_bf16x3_kernel<..., X6 = true> - three bf16 planes per operand split on the fly (split4x3), the six products
// lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi per 16-deep MFMA step in that order, K ascending - so for equal split-K chunks the two
// kernels produce identical bits.  What differs is the loop:
//
//   * 4 waves (2 x 2), each 128 x 64 of the tile (4 x 2 MFMA tiles of 32 x 32, 128 accumulator registers): 18 fragment reads per 48 MFMAs
//     instead of 12 per 24, W split once per 256 rows and A once per 128 columns.
//   * two LDS stages (2 x 72 KB).  The K-tile after next travels global -> registers while the next one is split (VALU) and written to
//     the other stage (ds_write_b64) IN THE ISSUE SLOTS BEHIND THE MFMAs of the current one, inside the same wave: a 32 x 32 x 16 MFMA
//     occupies the matrix pipe for 32 cycles, the wave's other instructions issue meanwhile (MI355X_MICROARCH: <= 5 per gap).  Per
//     MFMA the loop carries ~2.8 split instructions, 0.4 ds_read_b128, 0.4 ds_write_b64 and 0.13 global loads; the order is pinned
//     with sched_group_barrier.
//   * ONE barrier per K-tile, and the wave does not wait behind it: the MFMAs of the last step of tile t - 1 (fragments already in
//     registers) run while the first fragments of tile t are read.  Two fragment register sets (144 registers).
//
//   iteration t:   barrier | A(t): MFMA(t-1, step 1) || read frag(t, step 0) || stage units 0-5 of tile t+1, reload them with tile t+2
//                          | B(t): MFMA(t,   step 0) || read frag(t, step 1) || stage units 6-11 of tile t+1, reload them with tile t+2
//
// Hazards: stage (t+1)&1 is written during iteration t; its previous content (tile t-1) was last READ in B(t-1), before the barrier that
// opens iteration t (lgkmcnt(0) in front of it); tile t+1 is first read in A(t+1), behind the next barrier.
//
// Operand forms: dense A (M, K) fp32, or the implicit-GEMM view of a 3 x 3 / stride 1 convolution whose K-tiles lie inside one tap
// (Cin % 32 == 0: the tap of a tile is workgroup-uniform, addresses are a per-row register plus a scalar); optional pending normalisation of
// A (ANORM, as in the small-tile kernel); W fp32 (N, K).  K and the split-K chunk are multiples of 32 (host-checked): no K tails.
// Epilogue, split-K partials and the XCD tile order are those of the other kernels (rowwise_epilogue, 64-row statistics slabs).

namespace x6big {
constexpr int BM = 256, BKT = 32, NT = 256;
constexpr int ROWB = 64;                                   // bytes of a plane row (32 bf16), 16-byte chunks XOR-swizzled by (row >> 2) & 3
constexpr int PLANE_A = BM * ROWB;
constexpr int AU = BM / 32;                                // A staging units (one float4 per thread each): 8
constexpr int AN_MAXC = 512;
}  // namespace x6big

// BN = 128: waves 2 x 2, each 128 x 64 of the tile.  BN = 64 (narrow outputs: the 64-channel convolutions and stage-1 / stage-2 layers):
// waves 4 x 1, each 64 x 64 - 12 fragment reads per 24 MFMAs, W split once per 256 rows; the split of the A operand is then ~4.6 VALU
// instructions per MFMA, the loop is VALU-paced rather than matrix-paced.
template <bool ANORM, bool CONV, int BN = 128>
__global__ __launch_bounds__(256, 1) void gemm_x6_big_kernel(GemmArgs g) {
    using namespace x6big;
    static_assert(BN == 128 || BN == 64, "tile widths");
    constexpr int WM = BN == 128 ? 2 : 4, WN = 4 / WM;            // wave grid
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;          // MFMA tiles per wave: 4 x 2 / 2 x 2
    constexpr int PLANE_W = BN * ROWB, STAGE = 3 * (PLANE_A + PLANE_W);
    constexpr int WU = BN / 32, NU = AU + WU;                    // staging units of a K-tile: 8 + 4 / 8 + 2
    constexpr int TLD = BN + 4;
    static_assert(64 * TLD * 4 <= 2 * STAGE, "epilogue slab must fit in the stages");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * STAGE + (ANORM ? AN_MAXC * 8 : 0)];
    float *nsc = reinterpret_cast<float *>(lds_raw + 2 * STAGE), *nsh = nsc + AN_MAXC;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const BlockId bid = gemm_block_id(g);
    const int m0 = bid.y * BM, n0 = bid.x * BN;
    const int kbeg = bid.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int ntiles = (kend - kbeg) / BKT;
    const int lrow = tid >> 3, lk = (tid & 7) * 4;   // staging map: 8 lanes cover one 128-byte row slice, 32 rows per unit

    // ---- global addressing: workgroup-uniform base (scalar, advanced per tile) + per-thread 32-bit byte offsets that never change
    unsigned aoff[AU], woff[WU];
    unsigned vmask[CONV ? AU : 1];   // CONV: bit `tap` set = the input pixel under that tap lies inside the image
#pragma unroll
    for (int j = 0; j < WU; ++j) woff[j] = ((unsigned)(min(n0 + lrow + 32 * j, g.N - 1) - n0) * (unsigned)g.ldw + lk) * 4u;
    const char *wbase = reinterpret_cast<const char *>(g.W + (size_t)n0 * g.ldw + kbeg);
    const char *abase;
    if constexpr (CONV) {
        abase = reinterpret_cast<const char *>(g.A);
#pragma unroll
        for (int j = 0; j < AU; ++j) {
            const int r = min(m0 + lrow + 32 * j, g.M - 1);
            const int f = r / g.cv_Pout, pix = r - f * g.cv_Pout;
            const int yo = pix / g.cv_Wo, xo = pix - yo * g.cv_Wo;   // stride 1: output pixel = centre input pixel + pad - 1 ... (pad = 1: the same pixel)
            unsigned m = 0;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yi = yo - g.cv_pad + tap / 3, xi = xo - g.cv_pad + tap % 3;
                m |= ((unsigned)yi < (unsigned)g.cv_H && (unsigned)xi < (unsigned)g.cv_W) ? (1u << tap) : 0u;
            }
            vmask[j] = m;
            // offset of input pixel (yo, xo) of frame f - always inside the image (Ho <= H, Wo <= W for a stride-1 convolution with pad <= 1)
            aoff[j] = (((unsigned)f * (unsigned)(g.cv_H * g.cv_W) + (unsigned)(yo * g.cv_W + xo)) * (unsigned)g.lda + lk) * 4u;
        }
    } else {
        abase = reinterpret_cast<const char *>(g.A + (size_t)m0 * g.lda + kbeg);
#pragma unroll
        for (int j = 0; j < AU; ++j) aoff[j] = ((unsigned)(min(m0 + lrow + 32 * j, g.M - 1) - m0) * (unsigned)g.lda + lk) * 4u;
    }

    // ---- LDS addressing.  Staging: thread (lrow, lk) owns 8 bytes at k-byte 2 lk of rows lrow + 32 j; chunk = lk / 8, swizzled by the row
    const unsigned st_off = (unsigned)lrow * ROWB + (((((unsigned)lk >> 3) ^ ((unsigned)lrow >> 2)) & 3u) << 4) + (((unsigned)lk & 4u) << 1);
    // fragments: lane (li, lh) reads chunk 2 s + lh of row li (+ 32 i) of its wave's rows; the swizzle term depends on li only
    const int li = lane & 31, lh = lane >> 5;
    const unsigned swz = ((unsigned)li >> 2) & 3u;
    const unsigned fa_off = (unsigned)(wm * 32 * TM + li) * ROWB, fw_off = 3u * PLANE_A + (unsigned)(wn * 32 * TN + li) * ROWB;
    const unsigned co0 = (((unsigned)lh) ^ swz) << 4, co1 = ((2u + (unsigned)lh) ^ swz) << 4;

    f32x4 sr[NU];            // the K-tile in flight: raw fp32, one float4 per unit
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // conv: tap / channel position of the tile being LOADED (lt*) and of the tile being STAGED (st*), advanced incrementally (no division)
    int lt_tap = 0, lt_c = 0, st_tap = 0, st_c = 0;
    if constexpr (CONV) {
        lt_tap = st_tap = kbeg / g.cv_Cin;
        lt_c = st_c = kbeg - lt_tap * g.cv_Cin;
    }
    auto conv_advance = [&](int &tap, int &c) {
        c += BKT;
        if (c >= g.cv_Cin) { c -= g.cv_Cin; ++tap; }
        if (tap > 8) tap = 8;   // tiles past the range (clamped re-loads): stay inside the buffer
    };
    int lt = 0;   // index of the tile the next load unit reads (clamped to ntiles - 1)

    // one unit of the tile `lt`: unconditional load on an always valid address
    auto load_unit_to = [&](int u, f32x4 &dst) __attribute__((always_inline)) {
        if (u < AU) {
            if constexpr (CONV) {
                const int dy = lt_tap / 3, dx = lt_tap - 3 * dy;
                const int tapoff = ((dy - g.cv_pad) * g.cv_W + (dx - g.cv_pad)) * g.lda * 4;   // scalar
                const bool ok = (vmask[u] >> lt_tap) & 1u;
                const unsigned o = aoff[u] + (unsigned)(lt_c * 4) + (ok ? (unsigned)tapoff : 0u);
                dst = *reinterpret_cast<const f32x4 *>(abase + o);
            } else {
                dst = *reinterpret_cast<const f32x4 *>(abase + (size_t)lt * (BKT * 4) + aoff[u]);
            }
        } else {
            dst = *reinterpret_cast<const f32x4 *>(wbase + (size_t)lt * (BKT * 4) + woff[u - AU]);
        }
    };
    auto load_unit = [&](int u) __attribute__((always_inline)) { load_unit_to(u, sr[u]); };
    auto advance_load_tile = [&]() {
        if (lt + 1 < ntiles) {
            ++lt;
            if constexpr (CONV) conv_advance(lt_tap, lt_c);
        }
    };
    // split unit u of the staged tile into the planes of stage `sb` (byte offset of the stage)
    f32x4 nsc4, nsh4;   // ANORM: scale / shift of this thread's 4 channels for the tile being staged
    auto stage_unit = [&](int u, unsigned sb) {
        f32x4 v = sr[u];
        if (u < AU) {
            if constexpr (ANORM) {
                v = v * nsc4 + nsh4;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * g.an.slope);   // LeakyReLU, 0 <= slope <= 1: same bits as the select form
            }
            if constexpr (CONV) {
                const bool ok = (vmask[u] >> st_tap) & 1u;
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                v = ok ? v : zero;
            }
        }
        uint2 hi, mid, lo;
        split4x3(v, hi, mid, lo);
        const unsigned pl = u < AU ? PLANE_A : PLANE_W;
        unsigned char *p = lds_raw + sb + (u < AU ? 0u : 3u * PLANE_A) + st_off + (unsigned)((u < AU ? u : u - AU) * 32 * ROWB);
        *reinterpret_cast<uint2 *>(p) = hi;
        *reinterpret_cast<uint2 *>(p + pl) = mid;
        *reinterpret_cast<uint2 *>(p + 2 * pl) = lo;
    };
    auto stage_begin = [&](int tile_k0) {   // per-tile constants of the staged tile (k offset of the tile inside [kbeg, kend))
        if constexpr (ANORM) {
            const int ch = (CONV ? st_c : kbeg + min(tile_k0, (ntiles - 1) * BKT)) + lk;   // tiles past the range are staged but never read
            nsc4 = *reinterpret_cast<const f32x4 *>(nsc + ch);
            nsh4 = *reinterpret_cast<const f32x4 *>(nsh + ch);
        }
    };

    union Frag { uint4 u; bf16x8 v; };
    Frag fa0[TM][3], fw0[TN][3], fa1[TM][3], fw1[TN][3];   // two fragment sets: step 0 / step 1 of a tile; planes hi | mid | lo
    auto rd = [&](unsigned sb, unsigned co, Frag (&fa)[TM][3], Frag (&fw)[TN][3]) {
        const unsigned char *pa = lds_raw + sb + fa_off + co, *pw = lds_raw + sb + fw_off + co;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int p = 0; p < 3; ++p) fw[j][p].u = *reinterpret_cast<const uint4 *>(pw + p * PLANE_W + j * 32 * ROWB);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int p = 0; p < 3; ++p) fa[i][p].u = *reinterpret_cast<const uint4 *>(pa + p * PLANE_A + i * 32 * ROWB);
    };
    // the six products of one 16-deep step, product-major (consecutive MFMAs go to different accumulators), smallest terms first
    auto mm = [&](Frag (&fa)[TM][3], Frag (&fw)[TN][3]) {
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PW[6] = {0, 2, 1, 0, 1, 0};   // lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i][PA[q]].v, fw[j][PW[q]].v, acc[i][j], 0, 0, 0);
    };
    // Issue order of a phase: NMF MFMAs (one 16-deep step), the fragment reads of the next step, NU / 2 staging units (each ~22-40 VALU,
    // 3 ds_write_b64, 1 global load).  Per MFMA: VPM VALU; a fragment read behind the first MFMAs (the plane writes of the phase may
    // alias them for the compiler: reads first); a plane write / the re-load behind the later ones.
    auto pin_phase = [&](auto with_mfma) __attribute__((always_inline)) {
        constexpr int NMF = TM * TN * 6, NRD = (TM + TN) * 3, NWR = (NU / 2) * 3, NLD = NU / 2;
        constexpr int VBASE = (22 * (NU / 2) + NMF - 1) / NMF;   // VALU instructions of the split per MFMA: 3 (BN 128) / 5 (BN 64)
        constexpr int VPM = VBASE + (ANORM ? 1 : 0) + (CONV ? 1 : 0);
        constexpr int W0 = NMF / 8;                              // first MFMA with a plane write behind it
        constexpr int WSTEP = (NMF - W0 - 2) / NWR > 0 ? (NMF - W0 - 2) / NWR : 1;
        constexpr int LSTEP = NMF / NLD;
#pragma unroll
        for (int m = 0; m < NMF; ++m) {
            if constexpr (decltype(with_mfma)::value) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);                  // VALU
            if (m < NRD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // DS read
            if (m >= W0 && (m - W0) % WSTEP == 0 && (m - W0) / WSTEP < NWR) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
            if (m % LSTEP == LSTEP - 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);    // VMEM read
        }
    };

    // ---- prologue: tiles 0 and 1 -> registers in ONE round trip (the accumulators and fragments are not live yet: a second staging set is
    // free here), tile 0 -> stage 0
    f32x4 sr1[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) load_unit(u);
    advance_load_tile();
    if constexpr (!ANORM) {
#pragma unroll
        for (int u = 0; u < NU; ++u) load_unit_to(u, sr1[u]);
        advance_load_tile();
    }
    if constexpr (ANORM) {
        // statistics of this tile's frame -> scale / shift table in LDS: copied from the finalized vectors (cofi_norm_finalize) or folded
        // here from the producer's partials (the fold scratch lives in the still unused stages)
        const int f = g.an_rows > 0 ? m0 / g.an_rows : 0;
        if (g.an.scsh) {
            const float *src = g.an.scsh + (size_t)f * 2 * g.an.C;
            for (int c = tid * 4; c < g.an.C; c += NT * 4) {
                *reinterpret_cast<f32x4 *>(nsc + c) = *reinterpret_cast<const f32x4 *>(src + c);
                *reinterpret_cast<f32x4 *>(nsh + c) = *reinterpret_cast<const f32x4 *>(src + g.an.C + c);
            }
        } else {
            double *dred = reinterpret_cast<double *>(lds_raw);
            float *sstat = reinterpret_cast<float *>(lds_raw + NT * 32);
            fold_stat_table<NT, 6>(g.an.part + (size_t)f * g.an.nslab * g.an.tcols * 2, g.an.nslab, g.an.tcols, g.an.groups, g.an.count, g.an.eps,
                                   dred, sstat);
            norm_scale_shift<NT>(g.an, sstat, nsc, nsh);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < NU; ++u) load_unit_to(u, sr1[u]);   // behind the table (its fold wants the registers): overlaps the staging of tile 0
        advance_load_tile();
    }
    stage_begin(0);
#pragma unroll
    for (int u = 0; u < NU; ++u) stage_unit(u, 0u);
    if constexpr (CONV) conv_advance(st_tap, st_c);
#pragma unroll
    for (int u = 0; u < NU; ++u) sr[u] = sr1[u];
    __syncthreads();

    // ---- iteration 0: no MFMAs of a previous tile
    {
        rd(0u, co0, fa0, fw0);
        stage_begin(BKT);
#pragma unroll
        for (int u = 0; u < NU / 2; ++u) { stage_unit(u, (unsigned)STAGE); load_unit(u); }
        pin_phase(std::false_type{});
        __builtin_amdgcn_sched_barrier(0);
        rd(0u, co1, fa1, fw1);
        mm(fa0, fw0);
#pragma unroll
        for (int u = NU / 2; u < NU; ++u) { stage_unit(u, (unsigned)STAGE); load_unit(u); }
        pin_phase(std::true_type{});
        __builtin_amdgcn_sched_barrier(0);
        advance_load_tile();
        if constexpr (CONV) conv_advance(st_tap, st_c);
    }
    for (int t = 1; t < ntiles; ++t) {
        const unsigned sb = (t & 1) ? (unsigned)STAGE : 0u, so = (t & 1) ? 0u : (unsigned)STAGE;
        __syncthreads();   // tile t complete in stage sb (every wave's plane writes), tile t-1 no longer read
        // A(t)
        mm(fa1, fw1);
        rd(sb, co0, fa0, fw0);
        stage_begin((t + 1) * BKT);
#pragma unroll
        for (int u = 0; u < NU / 2; ++u) { stage_unit(u, so); load_unit(u); }
        pin_phase(std::true_type{});
        __builtin_amdgcn_sched_barrier(0);
        // B(t)
        mm(fa0, fw0);
        rd(sb, co1, fa1, fw1);
#pragma unroll
        for (int u = NU / 2; u < NU; ++u) { stage_unit(u, so); load_unit(u); }
        pin_phase(std::true_type{});
        __builtin_amdgcn_sched_barrier(0);
        advance_load_tile();
        if constexpr (CONV) conv_advance(st_tap, st_c);
    }
    if (ntiles > 0) mm(fa1, fw1);   // step 1 of the last tile

    const int lix = li, lhx = lh;
    if (g.ksplit > 1) {
        // raw partial sums straight from the D layout: row = (r&3) + 8*(r>>2) + 4*(lane>>5), col = lane&31
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int col = n0 + wn * 32 * TN + j * 32 + lix;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = m0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhx;
                    if (row < g.M && col < g.N) g.ws[((size_t)bid.z * g.M + row) * g.N + col] = acc[i][j][r];
                }
            }
        return;
    }
    // ---- epilogue in 64-row slabs through LDS
    float *lds = reinterpret_cast<float *>(lds_raw);
    auto slab_to_lds = [&](int h) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int rb = wm * TM + i;   // 32-row block of the tile held in acc[i][*]
            if ((rb >> 1) == h) {
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int rl = (rb & 1) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhx;
                        lds[rl * TLD + wn * 32 * TN + j * 32 + lix] = acc[i][j][r];
                    }
            }
        }
    };
    // (this tail is a copy of mfma32_tile_tail<..., LEAN = true> of gemm.hip, kept here because the shared form measured slower in this kernel:
    // a change to one has to be made in the other)
    // LEAN epilogue (no fused LayerNorm / L2 normalisation / sigmoid, whole float4 columns inside N, aligned output - every launch of the
    // forward that takes this kernel): straight-line code per slab, every decision uniform and taken once.  vmcnt counts stores as well as
    // loads: a load issued behind the stores of a slab makes its consumer wait for their round trip (and a wait the compiler places on a
    // path that happens to have no load at all still drains the stores) - four store round trips per tile otherwise.  So: bias and the 256
    // row divisors of the tile are loaded BEFORE the slab loop, which then holds no load at all; only a residual is loaded per slab, one
    // slab ahead of its use (before the stores of the slab in between).  Same operations in the same order as rowwise_epilogue: same bits.
    const bool vec_ok = ((g.N & 3) == 0) && ((g.ldc & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.C) & 15) == 0);
    const bool res_ok = !g.res || (((g.ldr & 3) == 0) && ((reinterpret_cast<uintptr_t>(g.res) & 15) == 0));
    if (!g.ln_gamma && !g.l2n && vec_ok && res_ok && n0 + BN <= g.N && g.act != COFI_ACT_SIGMOID) {
        constexpr int TPR = BN / 4, RPP = NT / TPR, NP = 64 / RPP, NS = BM / 64;   // 32 threads per row, 8 rows per pass, 8 passes per slab
        const int tc = tid % TPR, tr = tid / TPR;
        const int col = n0 + 4 * tc;
        const bool has_stats = g.colpart != nullptr;
        float bias4[4] = {0.f, 0.f, 0.f, 0.f};
        if (g.bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bias4[e] = g.bias[col + e];
        }
        float rd[NS][NP];
#pragma unroll
        for (int h = 0; h < NS; ++h)
#pragma unroll
            for (int p = 0; p < NP; ++p) rd[h][p] = 1.0f;
        if (g.rowdiv) {
#pragma unroll
            for (int h = 0; h < NS; ++h)
#pragma unroll
                for (int p = 0; p < NP; ++p) rd[h][p] = g.rowdiv[min(m0 + 64 * h + p * RPP + tr, g.M - 1)];   // rows past M are never stored
        }
        auto run = [&](auto with_res) __attribute__((always_inline)) {
            constexpr bool RES = decltype(with_res)::value;
            float rs[NP][4], rs_next[NP][4];
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int e = 0; e < 4; ++e) rs[p][e] = rs_next[p][e] = 0.f;
            auto load_res = [&](int h, float (&dst)[NP][4]) __attribute__((always_inline)) {
                if constexpr (RES) load_res_slab<NP, RPP>(g, m0 + 64 * h + tr, col, dst);
            };
            load_res(0, rs);
            __syncthreads();   // every wave is done with the operand stages
#pragma unroll
            for (int h = 0; h < NS; ++h) {
                const bool live = m0 + 64 * h < g.M;   // uniform: no statistics slab (and no rows) behind the last valid row
                if (live) slab_to_lds(h);
                __syncthreads();
                if (h + 1 < NS) load_res(h + 1, rs_next);
                float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
                if (live) {
                    float x[NP][4];
#pragma unroll
                    for (int p = 0; p < NP; ++p) {
                        const f32x4 t = *reinterpret_cast<const f32x4 *>(lds + (p * RPP + tr) * TLD + 4 * tc);
#pragma unroll
                        for (int e = 0; e < 4; ++e) x[p][e] = t[e];
                    }
                    epi_fast_apply<NP, RPP, RES>(g, x, bias4, rd[h], rs, col, m0 + 64 * h + tr, cs, cq);
                }
                if (has_stats) {   // uniform.  Fold of the RPP row phases in a fixed order, as rowwise_epilogue
                    __syncthreads();
                    if (live) colstat_fold<BN, RPP>(g, lds, cs, cq, (m0 >> 6) + h, n0, tr, tc);
                    else __syncthreads();
                }
                __syncthreads();
                if constexpr (RES) {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int e = 0; e < 4; ++e) rs[p][e] = rs_next[p][e];
                }
            }
        };
        if (g.res) run(std::true_type{});
        else run(std::false_type{});
        return;
    }
    // generic path: rowwise_epilogue per slab (loads its own operands)
    __syncthreads();
#pragma unroll
    for (int h = 0; h < BM / 64; ++h) {
        if (m0 + 64 * h >= g.M) break;   // uniform: no statistics slab (and no rows) behind the last valid row
        slab_to_lds(h);
        __syncthreads();
        rowwise_epilogue<64, BN, false, NT>(g, lds, TLD, m0 + 64 * h, n0, (m0 >> 6) + h, lds);
        __syncthreads();
    }
}
