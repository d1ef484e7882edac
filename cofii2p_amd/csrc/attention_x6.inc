// The attention kernel of attention.hip in the fp32-grade bf16 split arithmetic ("bf16x6", as gemm.hip): every fp32 operand - K, V, the
// scaled Q and the softmax weights P - is cut into three bf16 planes (hi / mid / lo, x == hi + mid + lo exactly) and each contraction
// is the six products lo.hi + hi.lo + mid.mid + mid.hi + hi.mid + hi.hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulation; the dropped
// terms are below 2^-24 of the product).  A 32 x 32 x 32 unit costs 2 x 6 MFMAs of 32 clocks instead of 16 of 64: the matrix pipe
// roof goes from 157 TF/s (fp32 instruction) to 2500 / 6 = 417 TF/s.  Included by attention.hip inside its anonymous namespace, below
// the skeleton it shares with the fp32 kernel (work decode, Q-scale fold, mask_tail, softmax_step, store_slot - see that file's
// header): same work partition (attn_layout), same slot output, same merge - this file holds the unit's arithmetic, the LDS image
// and staging that go with it, and the main-loop schedule.
//
// LDS image of a step: KPH K tiles + KPH V tiles, each as three bf16 planes of 32 rows x 64 B (+ 16 B pad: the 16-byte fragment reads
// of 8 consecutive rows fall into 8 different bank groups):
//   K plane row = key,  bf16 column c <-> head channel d = c             lane (key, h) reads columns 16 s + 8 h .. + 7 of k-step s
//   V plane row = d,    bf16 column 16 s + 8 h + i <-> key 16 s + 8 (i >> 2) + 4 h + (i & 3)   (V TRANSPOSED, keys in the order in
//                       which the D layout of S^T = K . Q^T holds them: lane (q, h) register r = 8 s + i is key 16 s + 8 (i>>2) + 4 h + (i&3))
// so P goes from the accumulator of the first chain to the B operand of the second one without leaving its lane (split in place),
// and O^T keeps "one query per lane" as in the fp32 kernel.  The staging threads do the splitting: a K thread loads 8 channels of a
// key (two float4), a V thread the 8 keys of one (tile, k-step, half) for one channel (8 dwords, 128-byte row segments per wave
// instruction) - each writes three 16-byte plane pieces.  One LDS buffer, two barriers per step: the unit's 12 fragment reads are
// complete at the first one (everything afterwards runs from registers); the next step's tiles - loaded to registers at the top of
// the step, in flight under the first chain - are split and written right behind it, so the staging registers are dead during
// the softmax and the second chain.  68 KB of LDS, 126 registers: two workgroups per CU.
//
// PRE (round 6): K / V arrive ALREADY SPLIT - cofi_attention_kv_planes wrote, once per (frame, head, key block), exactly the plane rows
// above (64-byte rows, dense): block image = [K hi | K mid | K lo | V^T hi | V^T mid | V^T lo], 6 x 2 KB.  With two query blocks per
// workgroup every (frame, head) is read by L / 64 workgroups, each of which otherwise repeats the split of the whole K / V (20 x at the
// KITTI shape: 72 of the ~290 vector instructions of a unit - the kernel is bound by vector issue, profiles/r05/attn_ablate.txt).  A step
// is then one contiguous 48 KB read: six 16-byte pieces per thread, copied to the padded LDS rows unchanged.  Inside a plane of the image the
// 128 pieces are stored COLUMN-major (piece (row r, 16-byte column c) at index 32 c + r): consecutive lanes then write consecutive rows of one
// column - 80 bytes apart, eight of them cover the 32 banks once - where row-major pieces (four lanes per 64-byte row) collide two ways.
namespace x6 {
constexpr int ROWB = 80;                  // bytes per plane row
constexpr int PT = 32 * ROWB;             // one plane of one tile
constexpr int KVB = 2 * KPH * 3 * PT;     // the step's image (61 440 B)
constexpr int IMG_PLANE = 32 * 64;        // a plane of the pre-split image: 32 rows x 64 B, dense
constexpr int IMG_BLOCK = 6 * IMG_PLANE;  // one key block: K hi | mid | lo | V^T hi | mid | lo (12 288 B)
}  // namespace x6

// K / V of one 32-key block -> the pre-split image (PRE above).  One workgroup per (key block, head, frame); threads 0..255: a K thread
// splits four channels of one key, a V thread four keys of one channel (the keys its 8-byte piece of the transposed row holds).
__global__ __launch_bounds__(256) void attention_kv_planes_kernel(const float *K, int ldk, const float *V, int ldv, int S, int H, unsigned char *img, int P) {
    using namespace x6;
    const int kb = blockIdx.x, h = blockIdx.y, f = blockIdx.z, tid = threadIdx.x;
    unsigned char *out = img + ((size_t)(f * H + h) * P + kb) * IMG_BLOCK;
    const size_t row0 = (size_t)f * S;
    {
        const int r = tid >> 3, c4 = tid & 7, key = kb * 32 + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (key < S) v = *reinterpret_cast<const f32x4 *>(K + (row0 + key) * ldk + h * D + 4 * c4);
        uint2 hi, mid, lo;
        cofi_split4x3(v, hi, mid, lo);
        unsigned char *p = out + ((c4 >> 1) * 32 + r) * 16 + (c4 & 1) * 8;   // 16-byte piece (row r, column c4 >> 1), pieces column-major (below)
        *reinterpret_cast<uint2 *>(p) = hi;
        *reinterpret_cast<uint2 *>(p + IMG_PLANE) = mid;
        *reinterpret_cast<uint2 *>(p + 2 * IMG_PLANE) = lo;
    }
    {
        // bf16 column 16 s + 8 hh + i of row d <-> key 16 s + 8 (i >> 2) + 4 hh + (i & 3): this thread's four columns i = 4 ih .. 4 ih + 3
        const int d = tid & 31, s = (tid >> 5) & 1, hh = (tid >> 6) & 1, ih = tid >> 7;
        const int key0 = kb * 32 + 16 * s + 8 * ih + 4 * hh;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = key0 + e < S ? V[(row0 + key0 + e) * ldv + h * D + d] : 0.f;
        uint2 hi, mid, lo;
        cofi_split4x3(v, hi, mid, lo);
        unsigned char *p = out + 3 * IMG_PLANE + ((2 * s + hh) * 32 + d) * 16 + 8 * ih;   // piece (row d, column 2 s + hh)
        *reinterpret_cast<uint2 *>(p) = hi;
        *reinterpret_cast<uint2 *>(p + IMG_PLANE) = mid;
        *reinterpret_cast<uint2 *>(p + 2 * IMG_PLANE) = lo;
    }
}

// DBG != 0 (instantiated only in builds with -DCOFI_ATTN_ABLATION, for tools/attn_ablate.py; results are wrong): 1 no global loads in the
// loop, 2 no barriers in the loop, 4 no softmax, 8 no staging split / LDS writes, 16 no second chain, 32 no first chain.
// Launch bounds "2 waves per SIMD": the kernel takes 126 registers either way (two workgroups per CU); compiled for 4 it measured the same.
template <int DBG, bool PRE>
__global__ __launch_bounds__(64 * NW, 2) void attention_x6_kernel(AttnArgs a) {
    using namespace x6;
    constexpr int SO = NW * 1024, SM = NW * 32, SP = 2 * NW * 32;
    static_assert(SO * 4 <= KVB, "the final states must fit in the staging buffer");
    constexpr int QLO = QG * 2 * 64 * 16;   // the lo plane of the two query blocks' Q fragments (used by 2 of a unit's 24 MFMAs: not worth 8 registers)
    __shared__ __attribute__((aligned(16))) unsigned char lds_raw[KVB + QLO + (2 * SM + 32 + SP) * 4];
    float *s_o = reinterpret_cast<float *>(lds_raw), *s_m = reinterpret_cast<float *>(lds_raw + KVB + QLO), *s_l = s_m + SM, *s_qs = s_l + SM, *s_part = s_qs + 32;
    unsigned char *s_qlo = lds_raw + KVB;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int ph = wave >> 1, qb_w = wave & 1;
    const AttnLayout &lay = a.lay;
    const AttnUnit u = attn_unit(blockIdx.x, gridDim.x, a);
    const int f = u.f, h = u.h, kb0 = u.kb0, nblk = u.nblk, nsteps = u.nsteps;
    const float *Kf = a.K + (size_t)f * a.S * a.ldk + h * D, *Vf = a.V + (size_t)f * a.S * a.ldv + h * D;

    // ---- staging.  K: thread (tile, key row, 8-channel piece); V: thread (channel, tile, k-step, half).  Buffer loads: rows past S
    // read as zero (masked in the softmax), tiles past the range read whatever follows (unused); one 32-bit add per load
    // instead of clamps and 64-bit address arithmetic.
    const int k_blk = tid >> 7, k_r = (tid >> 2) & 31, k_c8 = tid & 3;
    const int v_d = tid & 31, v_blk = tid >> 7, v_s = (tid >> 6) & 1, v_h = (tid >> 5) & 1;
    const __amdgpu_buffer_rsrc_t krs = PRE ? __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(a.kvimg) + (size_t)(f * a.H + h) * lay.P * IMG_BLOCK, 0,
                                                                              (unsigned)(lay.P * IMG_BLOCK), 0x00020000)
                                           : __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Kf), 0, (unsigned)(((size_t)(a.S - 1) * a.ldk + D) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(Vf), 0, (unsigned)(((size_t)(a.S - 1) * a.ldv + D) * 4), 0x00020000);
    const unsigned k_off = ((unsigned)(k_blk * 32 + k_r) * a.ldk + 8 * k_c8) * 4;
    const unsigned v_off = ((unsigned)(v_blk * 32 + 16 * v_s + 4 * v_h) * a.ldv + v_d) * 4;
    f32x4 sk[2], sv[2];
    u32x4 spre[PRE ? 6 : 1];   // PRE: the step's image is 3072 pieces of 16 bytes, piece tid + 512 j (j < 6) is this thread's
    auto stage_load = [&](int step) __attribute__((always_inline)) {
        if constexpr (PRE) {
            // (blocks past the pair's last one read as zero - the resource ends with the (frame, head) image - and are never multiplied)
            const unsigned o = (unsigned)(kb0 + step * KPH) * (unsigned)IMG_BLOCK + (unsigned)tid * 16u;
#pragma unroll
            for (int j = 0; j < 6; ++j) spre[j] = __builtin_amdgcn_raw_buffer_load_b128(krs, o + (unsigned)j * 8192u, 0, 0);
            return;
        }
        // (the scalar offset operand of a buffer load is NOT bounds checked: everything goes through the vector offset)
        const unsigned kv = k_off + (unsigned)(kb0 + step * KPH) * 32u * a.ldk * 4u, vv = v_off + (unsigned)(kb0 + step * KPH) * 32u * a.ldv * 4u;
        const u32x4 k0 = __builtin_amdgcn_raw_buffer_load_b128(krs, kv, 0, 0), k1 = __builtin_amdgcn_raw_buffer_load_b128(krs, kv + 16, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sk[0][e] = __uint_as_float(k0[e]);
            sk[1][e] = __uint_as_float(k1[e]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            sv[i >> 2][i & 3] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(vrs, vv + (unsigned)(8 * (i >> 2) + (i & 3)) * a.ldv * 4u, 0, 0));
    };
    // PRE: piece c = tid + 512 j lies in image plane u = c >> 7 = (tid >> 7) + 4 j of the step (block u / 6, K / V part (u % 6) / 3, plane u % 3),
    // row c & 31, 16-byte column (c & 127) >> 5 -> LDS tile ((part * KPH + block) * 3 + plane), padded rows
    const int pre_u0 = __builtin_amdgcn_readfirstlane(tid >> 7);
    const unsigned pre_rc = (unsigned)((tid & 31) * ROWB + ((tid & 127) >> 5) * 16);
    auto stage_store = [&]() __attribute__((always_inline)) {
        if constexpr (PRE) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int u = pre_u0 + 4 * j, blk = u / 6, r6 = u - 6 * blk, part = r6 / 3, plane = r6 - 3 * part;
                *reinterpret_cast<u32x4 *>(lds_raw + ((part * KPH + blk) * 3 + plane) * PT + pre_rc) = spre[j];
            }
            return;
        }
        uint2 h0, m0, l0, h1, m1, l1;
        cofi_split4x3(sk[0], h0, m0, l0);
        cofi_split4x3(sk[1], h1, m1, l1);
        unsigned char *p = lds_raw + (k_blk * 3) * PT + k_r * ROWB + 16 * k_c8;
        *reinterpret_cast<uint4 *>(p) = make_uint4(h0.x, h0.y, h1.x, h1.y);
        *reinterpret_cast<uint4 *>(p + PT) = make_uint4(m0.x, m0.y, m1.x, m1.y);
        *reinterpret_cast<uint4 *>(p + 2 * PT) = make_uint4(l0.x, l0.y, l1.x, l1.y);
        cofi_split4x3(sv[0], h0, m0, l0);
        cofi_split4x3(sv[1], h1, m1, l1);
        p = lds_raw + ((KPH + v_blk) * 3) * PT + v_d * ROWB + 32 * v_s + 16 * v_h;
        *reinterpret_cast<uint4 *>(p) = make_uint4(h0.x, h0.y, h1.x, h1.y);
        *reinterpret_cast<uint4 *>(p + PT) = make_uint4(m0.x, m0.y, m1.x, m1.y);
        *reinterpret_cast<uint4 *>(p + 2 * PT) = make_uint4(l0.x, l0.y, l1.x, l1.y);
    };
    // every wave's fragment reads of the step are complete (lgkmcnt only: the global loads of the next step stay in flight); the wait
    // is a builtin so that the compiler's own counter tracking sees it (it would otherwise put an s_waitcnt in front of each fragment's
    // first use - inside the MFMA chains)
    auto barrier_lds = [&]() __attribute__((always_inline)) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };

    // ---- prologue
    stage_load(0);
    f32x4 qraw[4];   // lane (q = li, h): Q[q][16 s + 8 h + 4 j + e] in qraw[2 s + j][e]
    const int qblk = u.qsb * QG + qb_w;          // this wave's query block; past the last one: idle wave (clamped loads, no slot)
    {
        const int q = min(qblk * 32 + li, a.L - 1);
        const float *qp = a.Q + ((size_t)f * a.L + q) * a.ldq + h * D + 8 * lh;
#pragma unroll
        for (int c = 0; c < 4; ++c) qraw[c] = *reinterpret_cast<const f32x4 *>(qp + 16 * (c >> 1) + 4 * (c & 1));
    }
    q_scale_partials(a, u, s_part);
    stage_store();
    q_scale_fold(a, u, s_part, s_qs);
    CofiFrag qp3[3][2];   // planes of q * colscale * softmax scale * log2(e): the B operand of S^T = K . Q^T ([2]: re-read from LDS per unit)
    const unsigned char *my_qlo = s_qlo + (qb_w * 2 * 64 + lane) * 16;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        f32x4 x[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const f32x4 sc = *reinterpret_cast<const f32x4 *>(&s_qs[16 * s + 8 * lh + 4 * j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[j][e] = (qraw[2 * s + j][e] * sc[e]) * a.scale_log2e;
        }
        uint2 h0, m0, l0, h1, m1, l1;
        cofi_split4x3(x[0], h0, m0, l0);
        cofi_split4x3(x[1], h1, m1, l1);
        qp3[0][s].u = make_uint4(h0.x, h0.y, h1.x, h1.y);
        qp3[1][s].u = make_uint4(m0.x, m0.y, m1.x, m1.y);
        if (ph == 0)   // wave-uniform
            *reinterpret_cast<uint4 *>(s_qlo + ((qb_w * 2 + s) * 64 + lane) * 16) = make_uint4(l0.x, l0.y, l1.x, l1.y);
    }
    __syncthreads();

    f32x16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;

    // the six products of a k-step, small terms first: (A plane, B plane) = (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi)
#define COFI_X6_CHAIN(acc, A, B, st)                                                           \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2][st].v, B[0][st].v, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0][st].v, B[2][st].v, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1][st].v, B[1][st].v, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1][st].v, B[0][st].v, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0][st].v, B[1][st].v, acc, 0, 0, 0);        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0][st].v, B[0][st].v, acc, 0, 0, 0);

    auto read_frags = [&](const unsigned char *tile, CofiFrag(&fr)[3][2]) __attribute__((always_inline)) {   // row li, columns 16 s + 8 h ..
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int st = 0; st < 2; ++st) fr[p][st].u = *reinterpret_cast<const uint4 *>(tile + p * PT + li * ROWB + 32 * st + 16 * lh);
    };
    auto split_p = [&](const f32x16 &p, CofiFrag(&pp)[3][2]) __attribute__((always_inline)) {   // P -> the B operand planes, in place
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            const f32x4 x0 = {p[8 * st], p[8 * st + 1], p[8 * st + 2], p[8 * st + 3]};
            const f32x4 x1 = {p[8 * st + 4], p[8 * st + 5], p[8 * st + 6], p[8 * st + 7]};
            uint2 h0, m0, l0, h1, m1, l1;
            cofi_split4x3(x0, h0, m0, l0);
            cofi_split4x3(x1, h1, m1, l1);
            pp[0][st].u = make_uint4(h0.x, h0.y, h1.x, h1.y);
            pp[1][st].u = make_uint4(m0.x, m0.y, m1.x, m1.y);
            pp[2][st].u = make_uint4(l0.x, l0.y, l1.x, l1.y);
        }
    };
    auto pv = [&](const f32x16 &p, const CofiFrag(&vf)[3][2]) __attribute__((always_inline)) {   // O^T += V^T . P^T
        CofiFrag pp[3][2];
        split_p(p, pp);
        __builtin_amdgcn_sched_barrier(0);   // bare chain (see front())
        COFI_X6_CHAIN(o, vf, pp, 0)
        COFI_X6_CHAIN(o, vf, pp, 1)
        __builtin_amdgcn_sched_barrier(0);
    };

    // ---- main loop: one unit per wave and step
    const bool tail_keys = (a.S & 31) != 0;
    // every step but the last has a unit for all four phases and a successor: one basic block without conditions
    f32x16 sC;
    CofiFrag vC[3][2];
    auto front = [&]() __attribute__((always_inline)) {   // S^T of this wave's tile; its V fragments
        CofiFrag kC[3][2];
        read_frags(lds_raw + (ph * 3) * PT, kC);
        qp3[2][0].u = *reinterpret_cast<const uint4 *>(my_qlo);
        qp3[2][1].u = *reinterpret_cast<const uint4 *>(my_qlo + 64 * 16);
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        sC = zero;   // (an inline constant of the first instruction)
        if constexpr (DBG & 32) {
#pragma unroll
            for (int r = 0; r < 16; ++r) sC[r] = __uint_as_float(kC[r % 3][r & 1].u[r & 3]) * __uint_as_float(qp3[r % 3][r & 1].u[r & 3]);
        } else {
            // A BARE chain: two MFMAs on the same accumulator issue 32 clocks apart only when nothing - no vector instruction, no
            // s_waitcnt - sits between them (+43 clocks for the first foreign issue slot, MI355X_MICROARCH.md): every operand is waited
            // for in front of the chain, the scheduler may not move anything into it; the vector work runs in the other waves of the SIMD
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
            __builtin_amdgcn_sched_barrier(0);
            COFI_X6_CHAIN(sC, kC, qp3, 0)
            COFI_X6_CHAIN(sC, kC, qp3, 1)
            __builtin_amdgcn_sched_barrier(0);
        }
        read_frags(lds_raw + ((KPH + ph) * 3) * PT, vC);
    };
    for (int t = 0; t + 1 < nsteps; ++t) {
        if constexpr (!(DBG & 1)) stage_load(t + 1);   // in flight under the first chain and the barrier
        front();
        if constexpr (!(DBG & 2)) barrier_lds();       // every wave holds its fragments of tile t in registers
        if constexpr (!(DBG & 8)) stage_store();       // the staging registers die before the softmax
        if constexpr (!(DBG & 4)) softmax_step(sC, o, m_run, l_run);         // (the partial last key block of a pair is never in these steps)
        if constexpr (!(DBG & 16)) pv(sC, vC);
        else o += sC;
        __builtin_amdgcn_sched_barrier(0);             // the second chain is issued before the barrier: its operands die in this step
        if constexpr (!(DBG & 2)) __syncthreads();     // tile t + 1 visible
    }
    {
        const int t = nsteps - 1, kb = kb0 + t * KPH + ph;
        const bool have = t * KPH + ph < nblk;   // wave-uniform
        if (have) front();
        barrier_lds();                           // the final states below re-use the staging image
        if (have) {
            if (tail_keys && kb == lay.P - 1) mask_tail(kb, a.S, lh, sC);
            softmax_step(sC, o, m_run, l_run);
            pv(sC, vC);
        }
    }
#undef COFI_X6_CHAIN

    store_slot(a, u, wave, li, lh, o, m_run, l_run, s_m, s_l, s_o);
}
