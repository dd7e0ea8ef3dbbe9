/*
 * alac_plan.h — the device-side launch plan of a decode and the scan that makes it from the sort-key histogram.
 * The scan is plain code over a count array, split into the part one thread does on its run of dispatch positions
 * and the part that needs the sums of the runs in front; k_sort.hip joins the two with a block-wide prefix sum, the
 * CPU suite (tests/host_sim/plan_sim.cpp) with a loop. Include behind alac_regular.h (the key ranges), with ALAC_DEV
 * defined.
 */
#ifndef ALAC_PLAN_H
#define ALAC_PLAN_H
#include <stdint.h>

#ifndef ALAC_DEV
#error "define ALAC_DEV before including alac_plan.h"
#endif

namespace alack {

/* device-side launch plan, rebuilt by every decode */
/* sort keys: 0..2047 regular packets (numU*32 + numV + KEY_WIDE, alac_regular.h); 2048 / 2049 irregular packets
 * (below). A workgroup holds packets of ONE key. */
constexpr uint32_t kKeys = alac::KEY_IRREGULAR + 2u;
constexpr uint32_t kKeyLegacy = alac::KEY_IRREGULAR;     /* decode_wave */
constexpr uint32_t kKeyScan = alac::KEY_IRREGULAR + 1u;  /* decode_wave<SCAN> + split pipeline */
struct Plan {
    uint32_t count[kKeys];     /* packets per key */
    uint32_t pkt_start[kKeys]; /* first index in perm[] */
    uint32_t spare[kKeys];     /* (the scatter's cursors until it took its ranks from the classify pass; nobody reads it: it
                                * keeps the fields behind it where the decode kernels' code expects them) */
    /* compact list of the non-empty keys in dispatch order (slowest first) */
    uint32_t nk;
    uint32_t list_key[kKeys];
    uint32_t list_wave0[kKeys]; /* first block id */
    uint32_t total_waves;
    uint32_t irr_waves;  /* waves of the irregular keys (>= KEY_IRREGULAR): they come first */
    uint32_t wide_waves; /* then those of the wide keys (KEY_WIDE..), then the narrow ones */
    /* the pair kernels (k_decode_body.inc; [0] narrow keys, [1] wide): workgroups admitted per CU so far and the
     * next item of the queue. Zeroed with the rest of the plan by every decode (k_sort.hip: sort_finish). */
    uint32_t gate[2][512];
    uint32_t balance[2][512]; /* per SIMD of the CU, a byte each: entropy waves - predictor waves placed there */
    uint32_t queue[2];
};
/* the words behind the lists that a decode starts from zero: gate, balance, queue */
constexpr uint32_t kPlanZeroDw = 2u * 512u + 2u * 512u + 2u;

/* Exclusive scan of the key histogram in dispatch order (highest key first: irregular packets, then the longest
 * predictors; a kernel ends when its last wave does, so the slowest waves get the lowest block ids). Dispatch
 * position q holds key kKeys - 1 - q. Packets per wave are a power of two, 1 << shift (alacgpu.hip: pick_ppw). */
struct PlanSums {
    uint32_t pkts, waves, keys, irr, wide; /* packets, waves, non-empty keys, waves of irregular / of wide keys */
};
ALAC_DEV uint32_t plan_waves_of(uint32_t c, uint32_t shift) { return (c + (1u << shift) - 1u) >> shift; }
/* the sums over the dispatch positions [q0, q0 + run) */
ALAC_DEV PlanSums plan_run_sums(const uint32_t* cnt, uint32_t q0, uint32_t run, uint32_t shift) {
    PlanSums s{0u, 0u, 0u, 0u, 0u};
    for (uint32_t q = q0; q < q0 + run && q < kKeys; ++q) {
        const uint32_t key = kKeys - 1u - q;
        const uint32_t c = cnt[key];
        const uint32_t cw = plan_waves_of(c, shift);
        s.pkts += c;
        s.waves += cw;
        s.keys += c ? 1u : 0u;
        s.irr += key >= alac::KEY_IRREGULAR ? cw : 0u;
        s.wide += (key >= alac::KEY_WIDE && key < alac::KEY_IRREGULAR) ? cw : 0u;
    }
    return s;
}
/* the plan's entries for the same positions, given the sums over all positions in front of q0 */
ALAC_DEV void plan_run_emit(const uint32_t* cnt, uint32_t q0, uint32_t run, uint32_t shift, PlanSums before, Plan* plan) {
    uint32_t ep = before.pkts, ew = before.waves, ez = before.keys;
    for (uint32_t q = q0; q < q0 + run && q < kKeys; ++q) {
        const uint32_t key = kKeys - 1u - q;
        const uint32_t c = cnt[key];
        plan->count[key] = c;
        plan->pkt_start[key] = ep;
        if (c) {
            plan->list_key[ez] = key;
            plan->list_wave0[ez] = ew;
            ++ez;
            ep += c;
            ew += plan_waves_of(c, shift);
        }
    }
}
/* ... and the totals, from the sums over all positions */
ALAC_DEV void plan_totals(PlanSums all, Plan* plan) {
    plan->nk = all.keys;
    plan->total_waves = all.waves;
    plan->irr_waves = all.irr;
    plan->wide_waves = all.wide;
}

} /* namespace alack */
#endif
