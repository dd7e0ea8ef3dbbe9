/* (included by k_dec*.hip with ALAC_DECODE_KERNEL / _WIDE / _DEPTH / _WAVES / _GATED / _ROLES set)
 * Regular packets: a workgroup of wavefronts per 64 packets with the SAME key (alac_duo.h), lane = packet in every wave:
 * ALAC_DECODE_ROLES 4 (narrow keys, k_dec*q.hip): entropy, predictor, writer and a spare wave; 2 (the wide keys and the
 * gated twin): entropy wave and predictor + PCM wave. ALAC_DECODE_WAVES waves per SIMD is the register budget.
 *
 * An item is one wave slot of the launch plan (64 packets of one key; the plan lists the slowest keys first). Two kinds
 * of kernel run them, and decode_mode() (alac_gpu.h) — evaluated on the device, where the number of items is known — says which:
 *
 *   ALAC_DECODE_GATED 0   one workgroup per item, placed by the hardware dispatcher, as many rounds as it takes. 34.5 KB
 *       of LDS per workgroup caps a CU at four, and up to 4 x CUs items the dispatcher spreads them exactly evenly.
 *       (16-bit: two such kernels, k_dec16q.hip and k_dec16l.hip with longer queue buffers; the host launches one of them in
 *       this shape, alacgpu.hip: long_chunks.)
 *   ALAC_DECODE_GATED 1   (16-bit only: its registers and 26 KB of LDS let six PAIRS share a CU) for item counts
 *       between the multiples of 4 x CUs, where the first kind would run a last, nearly empty round. As many
 *       workgroups as the device holds are launched; a workgroup asks its CU's gate for admission, the admitted ones
 *       (five or six per CU) take items until none is left. Left to itself the dispatcher fills CUs unevenly when more
 *       than the needed pairs fit (1 024 pairs on a device with room for 1 536: 2.80 ms instead of 2.45 ms), and the
 *       kernel ends with its slowest pair; so the gate counts pairs per CU, item j * CUs + c goes to the j-th pair on
 *       CU number c, and each pair picks which of its waves takes which role so that every SIMD hosts as many
 *       entropy as predictor waves. alacgpu_pair_placement() reads the outcome back.
 */
#ifndef ALAC_DECODE_ROLES
#define ALAC_DECODE_ROLES 2 /* waves per workgroup: entropy, predictor (+ PCM), and with 3 a writer of its own */
#endif
/* decode_mode() / pair_quota(): alac_gpu.h (the host reads the same decision back: alacgpu_last_dispatch) */

/* Which of a pair's two waves takes the entropy role (returns 1: the second one): whichever leaves the CU's SIMDs most
 * level. bal: the CU's word, (entropy waves - predictor waves) per SIMD, a byte each, biased by 128 (the memset's 0 = all
 * level). */
static __device__ __forceinline__ uint32_t pair_roles(uint32_t* bal, uint32_t simd0, uint32_t simd1) {
    uint32_t old = atomicAdd(bal, 0u), swap;
    for (;;) {
        const uint32_t cur = old ^ 0x80808080u;
        const int32_t d0 = (int32_t)((cur >> (8u * simd0)) & 255u) - 128, d1 = (int32_t)((cur >> (8u * simd1)) & 255u) - 128;
        /* straight: +1 on simd0, -1 on simd1; swapped: the reverse */
        swap = (simd0 != simd1 && d0 > d1) ? 1u : 0u;
        uint32_t nxt = cur;
        if (simd0 != simd1) {
            const uint32_t up = swap ? simd1 : simd0, dn = swap ? simd0 : simd1;
            nxt += 1u << (8u * up);
            nxt -= 1u << (8u * dn);
        }
        const uint32_t seen = atomicCAS(bal, old, nxt ^ 0x80808080u);
        if (seen == old) return swap;
        old = seen;
    }
}

/* The arguments are read from the kernel-argument segment where they are used (scalar loads, a few per item) instead of
 * being held in SGPRs across the whole item loop, where they would be spilled into VGPR lanes and read back inside the
 * decoding steps. */
typedef const PairArgs __attribute__((address_space(4))) * PairArgsPtr;
static __device__ __forceinline__ PairArgsPtr pair_args() {
    PairArgsPtr p = (PairArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p)); /* a fresh value every time: loads through it stay where they are written */
    return p;
}

/* one item = wave slot b of the plan: 64 packets (ppw of them when the batch is small) of one key */
static __device__ __forceinline__ void pair_item(PairArgsPtr ka, uint32_t b, uint32_t lane, uint32_t role, bool lanes_ok = false) {
    const Plan* plan = ka->plan;
    const uint32_t ppw = ka->ppw;
    const alac::DevCfg cfg{ka->cfg.frame_length, ka->cfg.bit_depth, ka->cfg.num_channels, ka->cfg.pb, ka->cfg.mb, ka->cfg.kb,
                           ka->cfg.bps, ka->cfg.aligned16};
    /* which key owns wave slot b: last list entry whose first wave is <= b (a handful of entries) */
    uint32_t e = 0;
    for (uint32_t t = 1; t < plan->nk; ++t)
        if (plan->list_wave0[t] <= b) e = t;
    const uint32_t key = plan->list_key[e];
#if ALAC_DECODE_ROLES == 4
    /* keys with a long predictor: waves 1 and 3 are predictor waves on several lanes per packet (alac_duo.h: duo_phase_lanes):
     * FOUR lanes while a wave slot holds at most 32 packets (batches of up to 16 383: pick_ppw), 16 of them to each of the two
     * waves, two lanes (32 packets each) with full slots; for every other key wave 3 has nothing to do */
    const bool lanes_on = lanes_ok && alac::duo_lanes_key((uint32_t)__builtin_amdgcn_readfirstlane((int)key), ka->cfg.num_channels == 2, ka->lanes_min);
    const uint32_t lpp = ppw <= 32u ? 4u : 2u;          /* lanes per packet */
    const uint32_t per_wave = kWave / lpp;              /* packets per predictor wave */
    if (role == 3u && (!lanes_on || ppw <= per_wave)) return;
    const bool lanes_wave = lanes_on && (role == 1u || role == 3u);
    const uint32_t lane_q = lane & (lpp - 1u);
    if (lanes_wave) lane = (role == 3u ? per_wave : 0u) + lane / lpp; /* from here on: the packet's column */
#endif
    const uint32_t idx = (b - plan->list_wave0[e]) * ppw + lane;
    const bool live = lane < ppw && idx < plan->count[key];
    const uint32_t pkt = live ? ka->perm[plan->pkt_start[key] + idx] : 0u;

    GpuWave wv;
    /* U tile: a column per lane (the decoders store without a branch, so lanes without a packet need cells too) */
    wv.u_tile = ka->scratch_u + (size_t)b * u_tile_cells(cfg.frame_length);
    wv.g_tile = nullptr;
    wv.ppw = ppw;
    wv.my_out = nullptr;
    wv.lane = lane;
    wv.wcnt = wv.flushed = wv.wpos = wv.fpos = 0;
#if defined(ALAC_SYNC_DIAG) && ALAC_DECODE_ROLES == 4
    /* (alac_gpu.h: kClaimDw) the first lane of a wave leaves its sums in the slot's record; of two predictor waves the first */
    wv.dg_waves = (lanes_on && ppw > per_wave) ? 4u : 3u;
    const uint64_t dg_t0 = __builtin_amdgcn_s_memtime();
#define ALAC_DG_RECORD(R)                                                       \
    if ((threadIdx.x & (kWave - 1u)) == 0u) {                                   \
        uint32_t* rec = pair_args()->claims + kClaimDw * b;                     \
        rec[4u * (R)] = wv.dg_wait[0];                                          \
        rec[4u * (R) + 1u] = wv.dg_last[0];                                     \
        rec[4u * (R) + 2u] = wv.dg_wait[1];                                     \
        rec[4u * (R) + 3u] = wv.dg_last[1];                                     \
        if ((R) == 0u) {                                                        \
            rec[14] = (uint32_t)(__builtin_amdgcn_s_memtime() - dg_t0);         \
            rec[15] = key;                                                      \
        }                                                                       \
    }
#else
#define ALAC_DG_RECORD(R)
#endif

    /* lanes without a packet read nothing (size 0) */
    const uint64_t off = live ? ka->offsets[pkt] : 0ull;
    const uint8_t* p = ka->blob + off;
    const uint32_t size = live ? ka->sizes[pkt] : 0u;
    const uint32_t avail = avail_of(ka->blob_bytes, off);
    uint8_t* o = ka->out + (size_t)pkt * ka->out_stride;
    uint32_t frames = 0;
    /* the key is wave-uniform (one key per workgroup): scalar branches pick the variant */
    const uint32_t ukey = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
#if ALAC_DECODE_ROLES >= 3
    constexpr bool EC = true;
    if (role == 2u) {
        /* the writer: few instructions per step, but the other two wait for it at every chunk's barrier: it goes first
         * whenever it has something to issue (at the lowest priority it starved: 24-bit pairs 820 ticks per step in the
         * writer against 430 in the other two) */
        __builtin_amdgcn_s_setprio(ALAC_PRIO_C);
        (void)alac::decode_regular_duo<GpuWave, alac::ROLE_C, ALAC_DECODE_WIDE, ALAC_DECODE_DEPTH, EC>(wv, cfg, ukey, live, p, size, avail, o, &frames);
        ALAC_DG_RECORD(2u)
        return;
    }
#else
    constexpr bool EC = false;
#endif
#if ALAC_DECODE_ROLES == 4
    if (lanes_wave) {
        /* the frame count of the packet in the same column of the other predictor wave (both waves take the entropy wave's
         * number of steps: the longest packet of all 64) */
        uint32_t ns_other = 0;
        {
            const uint32_t col2 = lane ^ per_wave, idx2 = (b - plan->list_wave0[e]) * ppw + col2;
            if (col2 < ppw && idx2 < plan->count[key]) {
                const uint32_t pkt2 = ka->perm[plan->pkt_start[key] + idx2];
                const uint64_t off2 = ka->offsets[pkt2];
                const alac::BitsT<false> b2{ka->blob + off2, ka->sizes[pkt2], avail_of(ka->blob_bytes, off2)};
                ns_other = (b2.get(19, 4) >> 3) ? b2.get(23, 32) : cfg.frame_length; /* decoder.go:232-235 */
            }
        }
        /* the longest waves of the workgroups that end last: they go first (like the long predictors of the wave pairs) */
        __builtin_amdgcn_s_setprio(ALAC_PRIO_B_LONG);
        if (lpp == 4u)
            (void)alac::decode_regular_duo<GpuWave, alac::ROLE_B, ALAC_DECODE_WIDE, ALAC_DECODE_DEPTH, EC, 4>(wv, cfg, ukey, live, p, size, avail, o, &frames,
                                                                                                           lane_q, ns_other);
        else
            (void)alac::decode_regular_duo<GpuWave, alac::ROLE_B, ALAC_DECODE_WIDE, ALAC_DECODE_DEPTH, EC, 2>(wv, cfg, ukey, live, p, size, avail, o, &frames,
                                                                                                           lane_q, ns_other);
        if (role == 1u) { ALAC_DG_RECORD(1u) }
        return;
    }
#endif
    if (role != 0u) {
        /* Issue priority goes to whichever wave is the longer one of its pair, and among pairs to the slowest (the
         * kernel ends with its slowest workgroup): role B grows by nine instructions per tap, role A does not, so
         * long predictors go ahead of everything, mid-length ones level with the entropy waves, short ones behind
         * (measured on the benchmark mix: 3.15 ms with the entropy waves on top, 2.73 ms this way). */
        const uint32_t na_max = max((ukey >> 5) & 31u, ukey & 31u);
        if (na_max > 8u && na_max != 31u) __builtin_amdgcn_s_setprio(ALAC_PRIO_B_LONG);
        else if (na_max >= 6u && na_max != 31u) __builtin_amdgcn_s_setprio(ALAC_PRIO_B_MID);
        else __builtin_amdgcn_s_setprio(ALAC_PRIO_B_SHORT);
        (void)alac::decode_regular_duo<GpuWave, alac::ROLE_B, ALAC_DECODE_WIDE, ALAC_DECODE_DEPTH, EC>(wv, cfg, ukey, live, p, size, avail, o, &frames);
        ALAC_DG_RECORD(1u)
        return;
    }
    /* the entropy chain is serial: it issues whenever it can, shorter predictor waves (many independent
     * instructions) fill the slots in between */
    {
        /* where the PCM writer runs in wave A (single channels, alac_duo.h) A is the longer wave of the pair */
        const bool cpe = cfg.num_channels == 2;
        if (!EC && !(ukey & alac::KEY_WIDE) && alac::duo_emit_in_a(cpe ? (ukey & 31u) : ((ukey >> 5) & 31u), cpe)) __builtin_amdgcn_s_setprio(3);
        else __builtin_amdgcn_s_setprio(ALAC_PRIO_A);
    }
    const int32_t st = alac::decode_regular_duo<GpuWave, alac::ROLE_A, ALAC_DECODE_WIDE, ALAC_DECODE_DEPTH, EC>(wv, cfg, ukey, live, p, size, avail, o, &frames);
    ALAC_DG_RECORD(0u)
    if (live) {
        PairArgsPtr kb = pair_args();
        kb->frames_out[pkt] = frames;
        kb->status[pkt] = st;
    }
}
#undef ALAC_DG_RECORD

#if !ALAC_DECODE_GATED

__global__ void __launch_bounds__(ALAC_DECODE_ROLES * kWave, ALAC_DECODE_WAVES) ALAC_DECODE_KERNEL(PairArgs) {
#if ALAC_DECODE_ROLES == 2
    /* the ungated pairs level the roles over the SIMDs too (pair_roles): 24-bit stereo, 65 536 packets: 3.59 -> 3.50 ms */
    __shared__ uint32_t s_swap, s_simd1;
    if (threadIdx.x == kWave) {
        uint32_t id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
        s_simd1 = (id >> 4) & 3u;
    }
    __syncthreads();
#endif
    PairArgsPtr ka = pair_args();
    Plan* plan = ka->plan;
    /* this kernel's half of the keys (narrow: 24-bit multiply-adds, wide: the literal 32-bit predictor) is a run of
     * consecutive wave slots: the plan lists irregular, wide, narrow */
    const uint32_t first = ALAC_DECODE_WIDE ? plan->irr_waves : plan->irr_waves + plan->wide_waves;
    const uint32_t items = ALAC_DECODE_WIDE ? plan->wide_waves : plan->total_waves - first;
    if (blockIdx.x >= items) return;
#if ALAC_DECODE_ROLES == 4
    if (decode_mode(items, ka->n_cu, ka->cap, ka->fit_force, ka->cfg.num_channels == 1u, ka->fit5 != 0u) != ka->fit) return; /* another launch's batch (alac_gpu.h: decode_mode) */
#endif
    uint32_t role = threadIdx.x >> 6;
    /* The workgroup's item of the list (slowest key first) is its number: the dispatcher hands workgroups b, b + CUs,
     * b + 2 CUs, b + 3 CUs to one CU (profiles/r03_final/placement/four_wave_65536.txt), so every CU gets one item from
     * each quarter of the list. Static deals that level the tap sums per CU further lose (experiments/static_deal.txt). */
    const uint32_t bid = blockIdx.x;
#if ALAC_DECODE_ROLES == 4
    /* Which of the four waves is the spare one (role 3: a second predictor wave for keys with long predictors, nothing
     * for the others). The four waves of a workgroup land on the CU's four SIMDs, and if every workgroup's LAST wave left
     * at once, the same SIMD of every CU would stand empty while the other three hold four waves each (65 536 packets:
     * 2.41 -> 2.73 ms). So the k-th workgroup to arrive on a CU (the CU's counter in the plan, as the gated kernel's gate)
     * spares its wave on SIMD k mod 4; the other three take entropy, predictor and writer role in wave order. */
    {
        __shared__ uint32_t s_simd[4], s_spare;
        if ((threadIdx.x & (kWave - 1u)) == 0u) {
            uint32_t id;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
            s_simd[threadIdx.x >> 6] = (id >> 4) & 3u;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t id, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            const uint32_t cu = ((xcc & 7u) << 6) | (((id >> 13) & 3u) << 4) | ((id >> 8) & 15u);
            const uint32_t k = atomicAdd(&plan->gate[ALAC_DECODE_WIDE][cu], 1u) & 3u;
            uint32_t spare = k; /* (waves that do not sit on four different SIMDs: by wave number) */
            for (uint32_t w = 0; w < 4u; ++w)
                if (s_simd[w] == k) spare = w;
            s_spare = spare;
#ifdef ALAC_SYNC_DIAG
            s_dg_arrive = 0u;
#endif
        }
        __syncthreads();
        const uint32_t rel = (role + 4u - s_spare) & 3u; /* 0: the spare wave */
        role = rel == 0u ? 3u : rel - 1u;
    }
#endif
#if ALAC_DECODE_ROLES == 2
    if (threadIdx.x == 0) {
        uint32_t id, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        const uint32_t cu = ((xcc & 7u) << 6) | (((id >> 13) & 3u) << 4) | ((id >> 8) & 15u);
        s_swap = pair_roles(&plan->balance[ALAC_DECODE_WIDE][cu], (id >> 4) & 3u, s_simd1);
    }
    __syncthreads();
    role ^= s_swap;
#endif
#if ALAC_DECODE_ROLES == 4 && defined(ALAC_DECODE_NO_LANES)
    /* (k_dec16l.hip: one predictor wave per workgroup; the constant takes duo_phase_lanes out of the kernel) */
    pair_item(ka, first + bid, threadIdx.x & (kWave - 1u), (uint32_t)__builtin_amdgcn_readfirstlane((int)role), false);
#elif ALAC_DECODE_ROLES == 4
    /* Two predictor waves for the long keys only while (nearly) every workgroup has a CU to itself (nine wave slots per eight CUs
     * (a partly filled slot per key comes on top of packets / 64): there the step of such a workgroup
     * shrinks with its longest wave (4 096 packets: 2.17 -> 1.56 ms; 16 384: 2.19 -> 2.09). On a fuller device the waves
     * share their SIMDs, the two predictor waves spend 164 instructions per step where the one spent 128, and the
     * workgroups that end last end later (32 768 packets: 2.19 -> 2.43 ms, 65 536: 2.42 -> 2.87). */
    pair_item(ka, first + bid, threadIdx.x & (kWave - 1u), (uint32_t)__builtin_amdgcn_readfirstlane((int)role), items <= ka->n_cu + ka->n_cu / 8u);
#else
    pair_item(ka, first + bid, threadIdx.x & (kWave - 1u), (uint32_t)__builtin_amdgcn_readfirstlane((int)role));
#endif
}

#else

/* next unclaimed item in list order, or none (>= items). Every item is claimed exactly once, by compare-and-swap of
 * its flag from 0 to the claimant's tag (include/alacgpu.h: alacgpu_pair_placement; bit 0: found by this sweep). */
static __device__ __forceinline__ uint32_t pair_sweep(Plan* plan, uint32_t* claims, uint32_t items, uint32_t tag) {
    for (;;) {
        const uint32_t t = atomicAdd(&plan->queue[ALAC_DECODE_WIDE], 1u);
        if (t >= items) return 0xffffffffu;
        if (atomicCAS(&claims[kClaimDw * t], 0u, tag | 1u) == 0u) return t;
    }
}

__global__ void __launch_bounds__(2 * kWave, ALAC_DECODE_WAVES) ALAC_DECODE_KERNEL(PairArgs) {
    __shared__ uint32_t s_item, s_tag, s_swap, s_simd1;
    uint32_t first, items;
    if (threadIdx.x == kWave) { /* the second wave tells the first which SIMD it is on (HW_ID [5:4]) */
        uint32_t id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
        s_simd1 = (id >> 4) & 3u;
    }
    __syncthreads();
    {
        PairArgsPtr ka = pair_args();
        Plan* plan = ka->plan;
        first = ALAC_DECODE_WIDE ? plan->irr_waves : plan->irr_waves + plan->wide_waves;
        items = ALAC_DECODE_WIDE ? plan->wide_waves : plan->total_waves - first;
        if (threadIdx.x == 0) {
            uint32_t item = 0xffffffffu, swap = 0u;
            const uint32_t n_cu = ka->n_cu;
            if (items != 0u && decode_mode(items, n_cu, ka->cap, ka->fit_force, ka->cfg.num_channels == 1u, ka->fit5 != 0u) == kModeGated) {
                /* HW_ID: simd [5:4], cu [11:8], se [14:13]; XCC_ID [3:0] (profiles/microbench/wave_census.hip) */
                uint32_t id, xcc;
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
                asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
                const uint32_t cu = ((xcc & 7u) << 6) | (((id >> 13) & 3u) << 4) | ((id >> 8) & 15u);
                const uint32_t simd0 = (id >> 4) & 3u, simd1 = s_simd1;
                const uint32_t quota = pair_quota(items, n_cu, ka->cap);
                uint32_t* claims = ka->claims + kClaimDw * first;
                const uint32_t j = atomicAdd(&plan->gate[ALAC_DECODE_WIDE][cu], 1u);
                if (j < quota) {
                    /* Which of the two waves takes the entropy role: whichever leaves the CU's SIMDs most level. The
                     * two roles issue very differently (A: one long dependent chain; B: many independent
                     * multiply-adds), and a SIMD that holds two of a kind is slower than one that holds one of each;
                     * where the waves of a workgroup land depends on what ran on the CU before (65 536 packets: up to
                     * 53 SIMD pairs of 512 with two of a kind, 2.80 ms; none, 2.65 ms). The CU's word holds (entropy
                     * waves - predictor waves) per SIMD, a byte each, biased by 128. */
                    swap = pair_roles(&plan->balance[ALAC_DECODE_WIDE][cu], simd0, simd1);
                    /* The j-th pair admitted on a CU starts with item j * n_cu + (the CU's number): the items are sorted
                     * slowest key first, so every CU gets one from each part of the list, and the pairs that arrive
                     * first (the oldest waves, which win the issue arbitration among equal priorities) get the slowest.
                     * The numbering is fixed per device (alacgpu.hip: cu_numbers; number c is on XCD c mod 8), so a CU
                     * works on the same U tiles in every decode. A CU the census missed takes what is left. */
                    const uint32_t r = ka->cu_number[cu] - 1u;
                    /* beyond four a CU the parts are dealt from the other end: a part that is not full then lands on
                     * the CUs whose first items are the least slow */
                    const uint32_t mine = j * n_cu + (j >= 4u ? n_cu - 1u - r : r);
                    const uint32_t tag = 0x80000000u | ((swap ? simd0 : simd1) << 19) | ((swap ? simd1 : simd0) << 17) | (cu << 8) |
                                         ((j < 15u ? j : 15u) << 4);
                    s_tag = tag;
                    /* a pair whose part of the list ends before its CU's turn has nothing to do: the items that are
                     * there all have a pair of their own on the way (taking one now would be taking a slow one
                     * from a CU that is still filling up) */
                    if (r >= n_cu) item = pair_sweep(plan, claims, items, tag);
                    else if (mine < items) item = atomicCAS(&claims[kClaimDw * mine], 0u, tag) == 0u ? mine : pair_sweep(plan, claims, items, tag);
                }
            }
            s_item = item;
            s_swap = swap;
        }
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & (kWave - 1u);
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)((threadIdx.x >> 6) ^ s_swap));
    for (;;) {
        const uint32_t item = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_item);
        if (item >= items) return;
        const uint64_t t0 = __builtin_amdgcn_s_memtime();
        pair_item(pair_args(), first + item, lane, role);
        /* whatever is left (more items than pairs at a time, or a pair that never came): in list order. Both waves are
         * through with the LDS queues (the last chunk's barrier). */
        __syncthreads();
        if (threadIdx.x == 0) {
            PairArgsPtr ka = pair_args();
            /* diagnostics (alacgpu_pair_placement): when the pair had the item */
            uint32_t* rec = ka->claims + kClaimDw * (first + item);
            rec[1] = (uint32_t)t0;
            rec[2] = (uint32_t)__builtin_amdgcn_s_memtime();
            s_item = pair_sweep(ka->plan, ka->claims + kClaimDw * first, items, s_tag);
        }
        __syncthreads();
    }
}

#endif
