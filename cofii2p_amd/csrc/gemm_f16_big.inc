// f16x3 contraction for the LARGE shapes: the 256 x 128 one-workgroup-per-CU loop of gemm_x6_big.inc in a THREE-product arithmetic
// (included by gemm.hip, inside its anonymous namespace).
//
// Arithmetic.  An fp32 operand x is carried as two fp16 planes of x * s, s a power of two:
//     hi = f16(x s)   (round to nearest even),   lo = f16(x s - hi)   (the residual is exact in fp32)
// hi + lo holds 22-24 significant bits of x s (|x s - hi - lo| <= 2^-22 |x s|, typically 2^-24), and the product is formed as
//     lo_a hi_w + hi_a lo_w + hi_a hi_w          on v_mfma_f32_32x32x16_f16, fp32 accumulation,
// dropping lo_a lo_w <= 2^-22 |a w|.  Against fp64 the result is as close as the exact-fp32 kernel's and the 6-term bf16 split's
// (tests/test_ops_gpu.py::test_gemm_f16x3_is_fp32_grade): their error is the fp32 ACCUMULATION (one rounding per product / per MFMA),
// which this kernel performs half as often as the 6-term split.  Half the matrix-pipe work per result of bf16x6 - the large
// contractions sit at the chip's power wall with six products (DESIGN.md 14.2).
//
// Range.  fp16 has 5 exponent bits; the lo plane sits 2^-11 below the hi plane, so x s must stay inside a window: below 65504
// (overflow) and high enough that the residuals are not flushed into the subnormal grid (absolute error 2^-25).  The scale is NOT a
// property the caller supplies and there is no global pre-pass: every workgroup keeps ONE running power-of-two scale per operand
// (its 256 x K panel of A, its 128 x K panel of W), chosen from the first K-tile so that the tile's largest |x s| lies in [2^13, 2^14).
// While a tile is split (with the current scale, optimistically) its largest scaled magnitude is tracked (one v_max3 per two values) and
// published per wave; behind the loop's one barrier every wave reads the four entries and, if the tile left the window
// (> 65504, or < 2^7 and non-zero), the workgroup LEAVES the pipelined loop and recomputes its output tile in a robust loop - one K-tile
// at a time: load, workgroup maximum, scale kept or re-chosen, accumulators multiplied by the ratio of the scales (a power of two: exact),
// split, MFMAs.  The decisions depend only on the data and the fixed tile order: results are reproducible bit for bit; a panel whose tile
// maxima stay within a factor 4 above / 64 below the tile that set the scale never leaves the fast loop
// (cofi_tune_f16x3_resplit_events counts the workgroups that did).  Rows whose entries are ALL far below their panel's largest
// entry lose relative accuracy (absolute error <= 2^-25 / s per element, i.e. <= 2^-32 of the tile maximum at the low end of the window,
// 2^-38 at its target) - the property of a per-panel scale; tests/test_ops_gpu.py holds the bound.
// The accumulators carry the factor sA sW; the epilogue (and the split-K partial store) multiplies by its reciprocal first - exact.
//
// Loop, tile geometry, LDS image (64-byte plane rows, 16-byte chunks XOR-swizzled by (row >> 2) & 3), operand forms (dense A,
// implicit 3 x 3 convolution, pending normalisation of A) and XCD tile order are those of gemm_x6_big_kernel, the tail behind the K loop
// is the shared one (gemm.hip, mfma32_tile_tail with its lean slab loop); two planes instead of three: 2 x 48 KB of LDS, 96 fragment registers.  The split of four values is 12 vector
// instructions (8 v_fma_mixlo/hi_f16: each half of hi and of lo is one fused multiply-add rounded to fp16 - the f16 operand of the residual
// read in place -, 2 more for the second hi half as an operand, 2 v_max3_f32) against 22 of the three-plane bf16 split; a static W arrives
// pre-split (WPRE below) and costs none.

namespace f16big {
constexpr int BM = 256, BN = 128, BKT = 32;
constexpr int ROWB = 64;                                   // bytes of a plane row (32 fp16), 16-byte chunks XOR-swizzled by (row >> 2) & 3
constexpr int PLANE_A = BM * ROWB, PLANE_W = BN * ROWB;
constexpr int STAGE = 2 * (PLANE_A + PLANE_W);             // hi | lo of A, hi | lo of W: 48 KB
constexpr int AN_MAXC = 512;
constexpr float WIN_HI = 65504.f, WIN_LO = 8.f;            // window of a tile's largest scaled magnitude
constexpr unsigned WIN_HI_BITS = 0x7c00u, WIN_LO_BITS = 0x4800u;   // ... as fp16 bit patterns of the hi plane: >= infinity / < 8
constexpr int TARGET_EXP = 11;                             // a (re)chosen scale puts the reference maximum into [2^11, 2^12): a tile may be 16-32 x larger or 256-512 x smaller
constexpr int SCOUTS = 8;                                  // K-tiles sampled (one staging unit each) for the reference maximum of the pipelined kernel
}  // namespace f16big

__device__ unsigned long long g_f16_resplit_events;   // diagnostic: workgroups that left the pipelined loop for the robust one (cofi_tune_f16x3_resplit_events)

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));

// power of two s with m * s in [2^14, 2^15); zero / subnormal / non-finite m: 1 (nothing to place, or nothing to save)
__device__ __forceinline__ float f16_scale_for(float m) {
    const unsigned e = (__float_as_uint(m) >> 23) & 0xffu;
    if (e == 0u || e == 255u) return 1.0f;
    int se = 127 + f16big::TARGET_EXP - ((int)e - 127);
    se = min(max(se, 27), 227);   // 2^-100 ... 2^100
    return __uint_as_float((unsigned)se << 23);
}

// full-wave maximum of unsigned values (DPP within rows of 16, row broadcasts across), returned to every lane
__device__ __forceinline__ unsigned wave_umax_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false));   // row_half_mirror
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false));   // row_mirror: every lane of a row holds the row's maximum
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));   // row_bcast15 into rows 1, 3
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));   // row_bcast31 into rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

typedef unsigned short u16x2v __attribute__((ext_vector_type(2)));

// Two values -> packed fp16 hi / lo of x * s; `m` tracks the largest |x| of the tile (unscaled; one v_max3_f32 per pair - publish() turns the
// wave's maximum into the fp16 bit pattern of its hi plane entry, the form the window is judged in).  Written so that each half is ONE
// instruction: hi = v_fma_mixlo/hi_f16(x, s, 0) (the fp32 product is exact - s is a power of two - and rounded to fp16 once, as
// v_cvt_pk_f16_f32 of x * s would), lo = v_fma_mixlo/hi_f16(x, s, -hi) (the residual is exact in fp32).  Six instructions per pair where
// multiply + pack + residual + pack + mask + packed maximum took eight; identical bits.  No inline asm: every instruction is visible to the
// scheduler that pins the loop's issue order.  gemm.hip is compiled with -fno-slp-vectorize (cofii2p_amd/build.py): the SLP pass would pack the
// pairs into v_pk_mul_f32 / v_pk_fma_f32 - slower beside MFMAs (DESIGN 14.6) - and lose the mix forms.
__device__ __forceinline__ void f16_split2_scaled(float x0, float x1, float s, unsigned &hi, unsigned &lo, float &m) {
#ifdef COFI_F16_SPLIT_MIX   // each half one v_fma_mixlo/hi_f16 (6 instructions per pair): measured SLOWER (profiles/r06/f16_probe_mix.txt: the partial
                            // register writes chain the halves), kept for the record
    f16x2v h, l;
    h[0] = (_Float16)__builtin_fmaf(x0, s, 0.0f);
    h[1] = (_Float16)__builtin_fmaf(x1, s, 0.0f);
    l[0] = (_Float16)__builtin_fmaf(x0, s, -(float)h[0]);
    l[1] = (_Float16)__builtin_fmaf(x1, s, -(float)h[1]);
#else
    const f16x2v h = __builtin_convertvector((f32x2){x0 * s, x1 * s}, f16x2v);   // v_cvt_pk_f16_f32 (RNE)
    const float r0 = __builtin_fmaf(x0, s, -(float)h[0]);                         // v_fma_mix_f32: x s - hi in one instruction, exact
    const float r1 = __builtin_fmaf(x1, s, -(float)h[1]);
    const f16x2v l = __builtin_convertvector((f32x2){r0, r1}, f16x2v);
#endif
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
    m = fmaxf(fmaxf(fabsf(x0), fabsf(x1)), m);   // v_max3_f32 m, |x0|, |x1|, m
}
// ... of values that carry their scale already (the normalising loader folds it into its scale / shift); `one` = 1.0f held opaque, so that
// the conversions stay the one-instruction mix forms.
__device__ __forceinline__ void f16_split2_prescaled(float v0, float v1, float one, unsigned &hi, unsigned &lo, float &m) {
    f16_split2_scaled(v0, v1, one, hi, lo, m);
}
// fp16 bit pattern of |v| (v >= 0): the hi plane entry of a value v = |x| s, as the window constants are written
__device__ __forceinline__ unsigned f16_bits_of(float v) {
    const _Float16 h = (_Float16)v;
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

// ROBUST = false: the pipelined kernel; a workgroup whose panel left the window writes 1 into its entry of g.fixflags (0 otherwise) and
// stores nothing.  ROBUST = true: the repair launch over the SAME grid behind it - a workgroup whose entry is 0 exits at once (the usual
// case: the whole launch is a few microseconds), one whose entry is 1 computes its output tile in the robust loop.  Two kernels, not two
// paths of one: with the robust loop inside the pipelined kernel the register allocator kept two copies of the 128 accumulators and
// moved them once per K-tile on the fast path.
// NW = waves per workgroup.  4: one wave per SIMD with all 512 registers, each 128 x 64 of the tile (the geometry of gemm_x6_big_kernel).
// 8: TWO waves per SIMD, each 64 x 64 of the tile with 256 registers: a lone in-order wave issues one instruction per ~9 cycles in this loop
// (dependent conversions, LDS and memory waits - the matrix pipe was 43 % busy with four waves), two waves fill each other's stalls.
// WPRE (COFI_GEMM_W_F16PRE): the static operand W arrives ALREADY SPLIT - every aligned group of four fp32 values of the (N, ldw) matrix is
// replaced, in place, by {hi0 hi1 hi2 hi3 | lo0 lo1 lo2 lo3} fp16 of w * s_panel (ops.pack_f16x3_weight), s_panel a power of two per 128-row
// panel stored behind the matrix (g.wscale) - so a staging unit is the same 16-byte load at the same address and its two plane pieces are the
// two halves of what it loaded: no conversion, no maximum tracking, no scouts for W (a third of the split work of a K-tile; every 128-row
// panel of W is otherwise split again by each of the M / 256 workgroups that read it).  The panel's scale covers the whole panel (it was
// chosen from its largest entry over all K), so W never leaves the window: the robust loop keeps it as well.
// BM_ = 128 (with NW = 4): a 128 x 128 tile, four waves of 64 x 64, 64 KB of LDS and <= 256 registers - TWO workgroups per CU whose barriers
// and waits are not aligned (one workgroup per CU leaves its SIMDs idle while all of its waves sit in front of the K-tile's barrier: 30 % of
// the wave cycles in the PMC passes of the 256-row form); a W tile is then staged once per 128 rows instead of 256, which costs nothing when
// it arrives pre-split.
template <bool ANORM, bool CONV, bool ROBUST, int NW, bool WPRE, int BM_ = 256>
__global__ __launch_bounds__(64 * NW, BM_ == 128 ? 2 : NW / 4) void gemm_f16_big_kernel(GemmArgs g) {
    using namespace f16big;
    constexpr int BM = BM_, PLANE_A = BM * ROWB, STAGE = 2 * (PLANE_A + PLANE_W);   // (shadow the 256-row constants of the namespace)
    constexpr int NT = 64 * NW, RPU = NT / 8;                  // threads; rows per staging unit (8 lanes cover one 128-byte row slice)
    constexpr int AU = BM / RPU, WU = BN / RPU, NU = AU + WU;  // staging units of a K-tile (one float4 per thread each): 8 + 4 / 4 + 2
    constexpr int WM = NW / 2, WN = 2, TM = BM / WM / 32, TN = BN / WN / 32;   // wave grid 2 x 2 (4 x 2 MFMA tiles of 32 x 32 per wave) / 4 x 2 (2 x 2)
    constexpr int FLAG_BYTES = 3 * NW * 8;                     // [2 parities + tile 0][waves]{largest |hi| of A, of W} as fp16 bit patterns
    constexpr int TLD = BN + 4;
    static_assert(64 * TLD * 4 <= 2 * STAGE, "epilogue slab must fit in the stages");
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * STAGE + FLAG_BYTES + (ANORM ? AN_MAXC * 8 : 0)];
    unsigned *flags = reinterpret_cast<unsigned *>(lds_raw + 2 * STAGE);
    float *nsc = reinterpret_cast<float *>(lds_raw + 2 * STAGE + FLAG_BYTES), *nsh = nsc + AN_MAXC;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const unsigned fix_id = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if constexpr (ROBUST) {
        if (g.fixflags[fix_id] == 0u) return;   // uniform
    }
    const BlockId bid = gemm_block_id(g);
    const int m0 = bid.y * BM, n0 = bid.x * BN;
    const int kbeg = bid.z * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const int ntiles = (kend - kbeg) / BKT;
    const int lrow = tid >> 3, lk = (tid & 7) * 4;   // staging map: 8 lanes cover one 128-byte row slice, RPU rows per unit

    // ---- global addressing: workgroup-uniform base (scalar, advanced per tile) + per-thread 32-bit byte offsets that never change
    unsigned aoff[AU], woff[WU];
    unsigned vmask[CONV ? AU : 1];   // CONV: bit `tap` set = the input pixel under that tap lies inside the image
#pragma unroll
    for (int j = 0; j < WU; ++j) woff[j] = ((unsigned)(min(n0 + lrow + RPU * j, g.N - 1) - n0) * (unsigned)g.ldw + lk) * 4u;
    const char *wbase = reinterpret_cast<const char *>(g.W + (size_t)n0 * g.ldw + kbeg);
    const char *abase;
    if constexpr (CONV) {
        abase = reinterpret_cast<const char *>(g.A);
#pragma unroll
        for (int j = 0; j < AU; ++j) {
            const int r = min(m0 + lrow + RPU * j, g.M - 1);
            const int f = r / g.cv_Pout, pix = r - f * g.cv_Pout;
            const int yo = pix / g.cv_Wo, xo = pix - yo * g.cv_Wo;
            unsigned m = 0;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int yi = yo - g.cv_pad + tap / 3, xi = xo - g.cv_pad + tap % 3;
                m |= ((unsigned)yi < (unsigned)g.cv_H && (unsigned)xi < (unsigned)g.cv_W) ? (1u << tap) : 0u;
            }
            vmask[j] = m;
            aoff[j] = (((unsigned)f * (unsigned)(g.cv_H * g.cv_W) + (unsigned)(yo * g.cv_W + xo)) * (unsigned)g.lda + lk) * 4u;
        }
    } else {
        abase = reinterpret_cast<const char *>(g.A + (size_t)m0 * g.lda + kbeg);
#pragma unroll
        for (int j = 0; j < AU; ++j) aoff[j] = ((unsigned)(min(m0 + lrow + RPU * j, g.M - 1) - m0) * (unsigned)g.lda + lk) * 4u;
    }

    // ---- LDS addressing (as gemm_x6_big_kernel)
    const unsigned st_off = (unsigned)lrow * ROWB + (((((unsigned)lk >> 3) ^ ((unsigned)lrow >> 2)) & 3u) << 4) + (((unsigned)lk & 4u) << 1);
    const int li = lane & 31, lh = lane >> 5;
    const unsigned swz = ((unsigned)li >> 2) & 3u;
    const unsigned fa_off = (unsigned)(wm * 32 * TM + li) * ROWB, fw_off = 2u * PLANE_A + (unsigned)(wn * 32 * TN + li) * ROWB;
    const unsigned co0 = (((unsigned)lh) ^ swz) << 4, co1 = ((2u + (unsigned)lh) ^ swz) << 4;

    f32x4 sr[NU];            // the K-tile in flight: raw fp32, one float4 per unit
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // running scales of the two operands (workgroup-uniform, held by every thread) and the maxima of the tile being split
    float sA = 1.0f, sW = 1.0f;
    float mA = 0.f, mW = 0.f;    // largest |x| (unscaled operand value; ANORM: the normalised, scaled one) of the tile being split
    float one = 1.0f;
    asm("" : "+v"(one));

    int lt_tap = 0, lt_c = 0, st_tap = 0, st_c = 0;
    if constexpr (CONV) {
        lt_tap = st_tap = kbeg / g.cv_Cin;
        lt_c = st_c = kbeg - lt_tap * g.cv_Cin;
    }
    auto conv_advance = [&](int &tap, int &c) {
        c += BKT;
        if (c >= g.cv_Cin) { c -= g.cv_Cin; ++tap; }
        if (tap > 8) tap = 8;
    };
    int lt = 0;

    // one unit of K-tile `t` (tap `tap`, first channel `c` for a convolution): unconditional load on an always valid address
    auto load_unit_at = [&](int u, int t, int tap, int c, f32x4 &dst) __attribute__((always_inline)) {
        if (u < AU) {
            if constexpr (CONV) {
                const int dy = tap / 3, dx = tap - 3 * dy;
                const int tapoff = ((dy - g.cv_pad) * g.cv_W + (dx - g.cv_pad)) * g.lda * 4;   // scalar
                const bool ok = (vmask[u] >> tap) & 1u;
                const unsigned o = aoff[u] + (unsigned)(c * 4) + (ok ? (unsigned)tapoff : 0u);
                dst = *reinterpret_cast<const f32x4 *>(abase + o);
            } else {
                dst = *reinterpret_cast<const f32x4 *>(abase + (size_t)t * (BKT * 4) + aoff[u]);
            }
        } else {
            dst = *reinterpret_cast<const f32x4 *>(wbase + (size_t)t * (BKT * 4) + woff[u - AU]);
        }
    };
    auto load_unit = [&](int u) __attribute__((always_inline)) { load_unit_at(u, lt, lt_tap, lt_c, sr[u]); };
    auto advance_load_tile = [&]() {
        if (lt + 1 < ntiles) {
            ++lt;
            if constexpr (CONV) conv_advance(lt_tap, lt_c);
        }
    };
    // ANORM: scale / shift of this thread's 4 channels for the tile being staged, the operand's running scale folded in
    f32x4 nsc4, nsh4;
    auto norm_consts = [&](int ch, float s, f32x4 &sc, f32x4 &sh) __attribute__((always_inline)) {
        sc = *reinterpret_cast<const f32x4 *>(nsc + ch) * s;
        sh = *reinterpret_cast<const f32x4 *>(nsh + ch) * s;
    };
    // split a raw unit into the planes of stage `sb` with the scales given; tracks the maxima in ma / mw
    auto split_store = [&](int u, f32x4 v, unsigned sb, int tap, const f32x4 &sc, const f32x4 &sh, float sa, float sw, float &ma, float &mw)
                           __attribute__((always_inline)) {
        uint2 hi, lo;
        if (u < AU) {
            if constexpr (ANORM) {
                v = v * sc + sh;   // = s * (y * scale + shift) exactly: the scale is a power of two
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * g.an.slope);   // LeakyReLU, 0 <= slope <= 1
            }
            if constexpr (CONV) {
                const bool ok = (vmask[u] >> tap) & 1u;
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                v = ok ? v : zero;
            }
            if constexpr (ANORM) {
                f16_split2_prescaled(v[0], v[1], one, hi.x, lo.x, ma);
                f16_split2_prescaled(v[2], v[3], one, hi.y, lo.y, ma);
            } else {
                f16_split2_scaled(v[0], v[1], sa, hi.x, lo.x, ma);
                f16_split2_scaled(v[2], v[3], sa, hi.y, lo.y, ma);
            }
        } else if constexpr (WPRE) {
            hi = make_uint2(__float_as_uint(v[0]), __float_as_uint(v[1]));
            lo = make_uint2(__float_as_uint(v[2]), __float_as_uint(v[3]));
        } else {
            f16_split2_scaled(v[0], v[1], sw, hi.x, lo.x, mw);
            f16_split2_scaled(v[2], v[3], sw, hi.y, lo.y, mw);
        }
        const unsigned pl = u < AU ? PLANE_A : PLANE_W;
        unsigned char *p = lds_raw + sb + (u < AU ? 0u : 2u * PLANE_A) + st_off + (unsigned)((u < AU ? u : u - AU) * RPU * ROWB);
        *reinterpret_cast<uint2 *>(p) = hi;
        *reinterpret_cast<uint2 *>(p + pl) = lo;
    };
    auto stage_unit = [&](int u, unsigned sb) __attribute__((always_inline)) { split_store(u, sr[u], sb, st_tap, nsc4, nsh4, sA, sW, mA, mW); };
    auto stage_begin = [&](int tile_k0) {   // per-tile constants of the staged tile (k offset of the tile inside [kbeg, kend))
        if constexpr (ANORM) {
            const int ch = (CONV ? st_c : kbeg + min(tile_k0, (ntiles - 1) * BKT)) + lk;   // tiles past the range are staged but never read
            norm_consts(ch, sA, nsc4, nsh4);
        }
    };
    // the maxima of the tile just split -> this wave's entry of the flag table (fp16 bit patterns of the largest |hi|)
    auto publish = [&](int parity) __attribute__((always_inline)) {
        // (non-negative floats order like their bit patterns; the wave's largest |x| times the scale it was split with -> its hi entry)
        const unsigned ua = f16_bits_of(__uint_as_float(wave_umax_u32(__float_as_uint(mA))) * (ANORM ? 1.0f : sA));
        const unsigned uw = WPRE ? 0u : f16_bits_of(__uint_as_float(wave_umax_u32(__float_as_uint(mW))) * sW);
        if (lane == 0) *reinterpret_cast<uint2 *>(flags + (parity * NW + wave) * 2) = make_uint2(ua, uw);
        mA = 0.f;
        mW = 0.f;
    };
    // largest entries of flag slot `slot` over the waves (every lane reads the same words: broadcast)
    auto slot_max = [&](int slot, unsigned &ua, unsigned &uw) __attribute__((always_inline)) {
        unsigned a = 0u, w = 0u;
#pragma unroll
        for (int q = 0; q < NW / 2; ++q) {
            const uint4 f = *reinterpret_cast<const uint4 *>(flags + slot * NW * 2 + 4 * q);
            a = max(a, max(f.x, f.z));
            w = max(w, max(f.y, f.w));
        }
        ua = (unsigned)__builtin_amdgcn_readfirstlane((int)a);
        uw = (unsigned)__builtin_amdgcn_readfirstlane((int)w);
    };
    auto read_flags = [&](int slot, float &fa, float &fw) __attribute__((always_inline)) {   // ... holding fp32 bit patterns (prologue, robust loop)
        unsigned ua, uw;
        slot_max(slot, ua, uw);
        fa = __uint_as_float(ua);
        fw = __uint_as_float(uw);
    };

    union Frag { uint4 u; f16x8 v; };
    Frag fa0[TM][2], fw0[TN][2], fa1[TM][2], fw1[TN][2];   // two fragment sets: step 0 / step 1 of a tile; planes hi | lo
    auto rd = [&](unsigned sb, unsigned co, Frag (&fa)[TM][2], Frag (&fw)[TN][2]) {
        const unsigned char *pa = lds_raw + sb + fa_off + co, *pw = lds_raw + sb + fw_off + co;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int p = 0; p < 2; ++p) fw[j][p].u = *reinterpret_cast<const uint4 *>(pw + p * PLANE_W + j * 32 * ROWB);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int p = 0; p < 2; ++p) fa[i][p].u = *reinterpret_cast<const uint4 *>(pa + p * PLANE_A + i * 32 * ROWB);
    };
    // the three products of one 16-deep step, product-major (consecutive MFMAs go to different accumulators), smallest terms first
    auto mm = [&](Frag (&fa)[TM][2], Frag (&fw)[TN][2]) {
        constexpr int PA[3] = {1, 0, 0}, PW[3] = {0, 1, 0};   // lo*hi, hi*lo, hi*hi
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i][PA[q]].v, fw[j][PW[q]].v, acc[i][j], 0, 0, 0);
    };
    // Issue order of a phase: NMF MFMAs (one 16-deep step); behind each of them VPM vector instructions of the NU / 2 staging units (split
    // 12, maxima 2, address 1-2; the normalising loader 16 more, the convolution's mask 4-5); the fragment reads of the next step behind the
    // first NRD MFMAs; the plane writes and the re-loads of the units behind the later ones - the writes may alias the reads for the
    // compiler, so a write slot among the read slots cannot be filled, and a pipeline with an unfillable slot falls apart into "all vector
    // work, then all MFMAs" (measured: matrix pipe 38 % busy).
    auto pin_phase = [&](auto with_mfma) __attribute__((always_inline)) {
        constexpr int NMF = TM * TN * 3, NRD = (TM + TN) * 2, NUH = NU / 2;
        constexpr int VUNIT = 13 + (ANORM ? 16 : 0) + (CONV ? 5 : 0);
        constexpr int VPM = (VUNIT * NUH + 16 + NMF - 1) / NMF;   // (WPRE: the W units of the second phase carry ~2 instead of 15 - the slots stay, partly empty)
        constexpr int WSTEP = (NMF - NRD) / NUH > 0 ? (NMF - NRD) / NUH : 1;
#pragma unroll
        for (int m = 0; m < NMF; ++m) {
            if constexpr (decltype(with_mfma)::value) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);                  // VALU
            if (m < NRD) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);       // DS read
            if (m >= NRD && (m - NRD) % WSTEP == 0 && (m - NRD) / WSTEP < NUH) {
                __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write: both planes of a unit (one ds_write2st64_b64)
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read: the unit's registers are free
            }
        }
    };

    // ANORM: statistics of this tile's frame -> scale / shift table in LDS: copied from the finalized vectors (cofi_norm_finalize) or folded
    // here from the producer's partials (the fold scratch lives in the still unused stages); ends on a barrier
    auto load_norm_table = [&]() {
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
    };

    if constexpr (!ROBUST) {
        // ---- prologue: tiles 0 and 1 -> registers in ONE round trip, the scales from tile 0, tile 0 -> stage 0
        f32x4 sr1[NU];
    #pragma unroll
        for (int u = 0; u < NU; ++u) load_unit(u);
        advance_load_tile();
        if constexpr (!ANORM) {
    #pragma unroll
            for (int u = 0; u < NU; ++u) load_unit_at(u, lt, lt_tap, lt_c, sr1[u]);
            advance_load_tile();
        }
        if constexpr (ANORM) {
            load_norm_table();
    #pragma unroll
            for (int u = 0; u < NU; ++u) load_unit_at(u, lt, lt_tap, lt_c, sr1[u]);
            advance_load_tile();
        }
        {
            // The reference maximum of the panel: all of tile 0 and one staging unit (32 rows x 32 k per operand) of SCOUTS K-tiles spread over
            // the K range, as the MFMAs will see them (A: normalised / masked), unscaled.  A panel whose magnitude changes along K - the
            // channel blocks of a concatenation, the kernel points of a KPConv aggregate - is placed by its LARGEST block, so the smaller
            // ones sit lower in the window instead of the larger ones overflowing it.
            float pa = 0.f, pw = 0.f;
            auto seen_a = [&](f32x4 v, int u, int tap, int ch) __attribute__((always_inline)) {
                if constexpr (ANORM) {
                    f32x4 sc1, sh1;
                    norm_consts(ch + lk, 1.0f, sc1, sh1);
                    v = v * sc1 + sh1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * g.an.slope);
                }
                if constexpr (CONV) {
                    const bool ok = (vmask[u] >> tap) & 1u;
                    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                    v = ok ? v : zero;
                }
                asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pa) : "v"(v[0]), "v"(v[1]));
                asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pa) : "v"(v[2]), "v"(v[3]));
            };
            {
                f32x4 sca[SCOUTS], scw[SCOUTS];
                int stp[SCOUTS], sch[SCOUTS];
#pragma unroll
                for (int j = 1; j < SCOUTS; ++j) {
                    const int tj = (int)(((long)j * ntiles) / SCOUTS);
                    int tap = 0, c = 0;
                    if constexpr (CONV) {
                        const int kk = kbeg + tj * BKT;
                        tap = kk / g.cv_Cin;
                        c = kk - tap * g.cv_Cin;
                    }
                    stp[j] = tap;
                    sch[j] = CONV ? c : kbeg + tj * BKT;
                    load_unit_at(j % AU, tj, tap, c, sca[j]);
                    if constexpr (!WPRE) load_unit_at(AU + j % WU, tj, tap, c, scw[j]);
                }
#pragma unroll
                for (int j = 1; j < SCOUTS; ++j) {
                    seen_a(sca[j], j % AU, stp[j], sch[j]);
                    if constexpr (!WPRE) {
                        asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pw) : "v"(scw[j][0]), "v"(scw[j][1]));
                        asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pw) : "v"(scw[j][2]), "v"(scw[j][3]));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if (u < AU) {
                    seen_a(sr[u], u, st_tap, CONV ? st_c : kbeg);
                } else if constexpr (!WPRE) {
                    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pw) : "v"(sr[u][0]), "v"(sr[u][1]));
                    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pw) : "v"(sr[u][2]), "v"(sr[u][3]));
                }
            }
            const unsigned ua = wave_umax_u32(__float_as_uint(pa)), uw = wave_umax_u32(__float_as_uint(pw));
            if (lane == 0) *reinterpret_cast<uint2 *>(flags + wave * 2) = make_uint2(ua, uw);
            __syncthreads();
            float fa, fw;
            read_flags(0, fa, fw);
            sA = f16_scale_for(fa);
            sW = WPRE ? g.wscale[bid.x] : f16_scale_for(fw);
        }
        stage_begin(0);
    #pragma unroll
        for (int u = 0; u < NU; ++u) stage_unit(u, 0u);
        publish(2);   // tile 0 cannot overflow (it is part of the reference maximum) but it may lie BELOW the window: judged in front of the loop
        if constexpr (CONV) conv_advance(st_tap, st_c);
    #pragma unroll
        for (int u = 0; u < NU; ++u) sr[u] = sr1[u];
        __syncthreads();

        bool fallback;
        {
            unsigned ua, uw;
            slot_max(2, ua, uw);
            fallback = (ua > 0u && ua < WIN_LO_BITS) || (uw > 0u && uw < WIN_LO_BITS);
        }
        // ---- iteration 0: no MFMAs of a previous tile
        if (!fallback) {
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
            publish(1);
            advance_load_tile();
            if constexpr (CONV) conv_advance(st_tap, st_c);
        }
        // ---- the pipelined loop.  The flag entries of tile t (split during iteration t - 1) are read behind the barrier and judged at the END of
        // the iteration: a tile outside the window makes the workgroup leave this loop (what it accumulated meanwhile - possibly from planes
        // with infinities - is discarded) and recompute its output tile in the robust loop below.  Nothing in here redefines the accumulators
        // outside the two MFMA chains: the loop stays one basic block (a mid-iteration repair path cost 128 accumulator copies per K-tile).
        for (int t = 1; t < ntiles && !fallback; ++t) {
            const unsigned sb = (t & 1) ? (unsigned)STAGE : 0u, so = (t & 1) ? 0u : (unsigned)STAGE;
            __syncthreads();   // tile t complete in stage sb (every wave's plane writes and flag entries), tile t-1 no longer read
            uint4 fl[NW / 2];   // tile t's flag entries: read now, judged at the end of the iteration
#pragma unroll
            for (int q = 0; q < NW / 2; ++q) fl[q] = *reinterpret_cast<const uint4 *>(flags + (t & 1) * NW * 2 + 4 * q);
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
            publish((t + 1) & 1);
            advance_load_tile();
            if constexpr (CONV) conv_advance(st_tap, st_c);
            {
                unsigned xa = 0u, xw = 0u;
#pragma unroll
                for (int q = 0; q < NW / 2; ++q) {
                    xa = max(xa, max(fl[q].x, fl[q].z));
                    xw = max(xw, max(fl[q].y, fl[q].w));
                }
                const unsigned ua = (unsigned)__builtin_amdgcn_readfirstlane((int)xa), uw = (unsigned)__builtin_amdgcn_readfirstlane((int)xw);
                const bool badA = ua >= WIN_HI_BITS || (ua > 0u && ua < WIN_LO_BITS), badW = uw >= WIN_HI_BITS || (uw > 0u && uw < WIN_LO_BITS);
                if (__builtin_expect(badA || badW, 0)) {
                    fallback = true;
                    break;
                }
            }
        }
        if (tid == 0) g.fixflags[fix_id] = fallback ? 1u : 0u;   // read by the repair launch behind this one
        if (fallback) return;                                      // uniform: this tile is the repair launch's
        if (ntiles > 0) mm(fa1, fw1);   // step 1 of the last tile
    } else {
        // ---- robust loop (rare): the whole K range again, one tile at a time - load, workgroup maximum, scale decision, split, MFMAs - with
        // a scale that follows the data: kept while the tile's largest scaled magnitude stays inside the window, re-chosen otherwise, the
        // accumulators multiplied by the ratio (a power of two: exact).  Deterministic like the fast loop: only the data decide.
        if (tid == 0) atomicAdd(&g_f16_resplit_events, 1ull);
        if constexpr (ANORM) load_norm_table();
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        int tap = 0, c = 0;
        if constexpr (CONV) {
            tap = kbeg / g.cv_Cin;
            c = kbeg - tap * g.cv_Cin;
        }
        f32x4 raw[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) load_unit_at(u, 0, tap, c, raw[u]);
        float sa = 1.0f, sw = WPRE ? g.wscale[bid.x] : 1.0f;
        for (int t = 0; t < ntiles; ++t) {
            f32x4 sc1, sh1;
            if constexpr (ANORM) norm_consts((CONV ? c : kbeg + t * BKT) + lk, 1.0f, sc1, sh1);
            float pa = 0.f, pw = 0.f;
#pragma unroll
            for (int u = 0; u < NU; ++u) {   // the values the MFMAs will see (A: normalised / masked), unscaled, and their maxima
                f32x4 v = raw[u];
                if (u < AU) {
                    if constexpr (ANORM) {
                        v = v * sc1 + sh1;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], v[e] * g.an.slope);
                    }
                    if constexpr (CONV) {
                        const bool ok = (vmask[u] >> tap) & 1u;
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                        v = ok ? v : zero;
                    }
                    raw[u] = v;
                    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pa) : "v"(v[0]), "v"(v[1]));
                    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pa) : "v"(v[2]), "v"(v[3]));
                } else if constexpr (!WPRE) {
                    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pw) : "v"(v[0]), "v"(v[1]));
                    asm("v_max3_f32 %0, |%1|, |%2|, %0" : "+v"(pw) : "v"(v[2]), "v"(v[3]));
                }
            }
            {
                const unsigned ua = wave_umax_u32(__float_as_uint(pa)), uw = wave_umax_u32(__float_as_uint(pw));
                if (lane == 0) *reinterpret_cast<uint2 *>(flags + wave * 2) = make_uint2(ua, uw);
            }
            __syncthreads();   // maxima of every wave; the fragment reads of tile t - 1 are done
            float fa, fw;
            read_flags(0, fa, fw);
            float na = sa, nw = sw;
            {
                const float ma = fa * sa, mw = fw * sw;
                if (t == 0 || !(ma <= WIN_HI) || (ma > 0.f && ma < WIN_LO)) na = f16_scale_for(fa);
                if constexpr (!WPRE)
                    if (t == 0 || !(mw <= WIN_HI) || (mw > 0.f && mw < WIN_LO)) nw = f16_scale_for(fw);
            }
            if (t > 0 && (na != sa || nw != sw)) {
                const float ratio = (na / sa) * (nw / sw);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] *= ratio;
            }
            sa = na;
            sw = nw;
            float dm = 0.f;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                uint2 hi, lo;
                const float su = u < AU ? sa : sw;
                if (WPRE && u >= AU) {
                    hi = make_uint2(__float_as_uint(raw[u][0]), __float_as_uint(raw[u][1]));
                    lo = make_uint2(__float_as_uint(raw[u][2]), __float_as_uint(raw[u][3]));
                } else {
                    f16_split2_scaled(raw[u][0], raw[u][1], su, hi.x, lo.x, dm);
                    f16_split2_scaled(raw[u][2], raw[u][3], su, hi.y, lo.y, dm);
                }
                const unsigned pl = u < AU ? PLANE_A : PLANE_W;
                unsigned char *p = lds_raw + (u < AU ? 0u : 2u * PLANE_A) + st_off + (unsigned)((u < AU ? u : u - AU) * RPU * ROWB);
                *reinterpret_cast<uint2 *>(p) = hi;
                *reinterpret_cast<uint2 *>(p + pl) = lo;
            }
            if (t + 1 < ntiles) {   // the next tile travels while this one is multiplied
                if constexpr (CONV) conv_advance(tap, c);
#pragma unroll
                for (int u = 0; u < NU; ++u) load_unit_at(u, t + 1, tap, c, raw[u]);
            }
            __syncthreads();   // planes of tile t
            rd(0u, co0, fa0, fw0);
            rd(0u, co1, fa1, fw1);
            mm(fa0, fw0);
            mm(fa1, fw1);
        }
        sA = sa;
        sW = sw;
    }

    // the accumulators carry sA * sW: take it out first (a power of two)
    {
        const float inv = (1.0f / sA) * (1.0f / sW);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] *= inv;
    }

    // ---- split-K partials, or the epilogue in 64-row slabs through LDS (lean where its conditions hold)
    mfma32_tile_tail<BM, BN, TM, TN, NT, true>(g, acc, reinterpret_cast<float *>(lds_raw), bid.z, m0, n0, wm, wn, li, lh, tid);
}
