/*
 * plan_sim.cpp — TEST-ONLY host build of the launch plan's scan (saprobe-alac_amd/csrc/alac_plan.h, the exact text the
 * sort kernels of k_sort.hip are built from). The device joins the per-thread runs with a block-wide prefix sum over 256
 * threads; here a loop does, over any number of "threads", so the CPU suite can compare the plan with numpy. Never linked
 * into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#define ALAC_DEV inline
#include "../../saprobe-alac_amd/csrc/alac_wave.h"
#include "../../saprobe-alac_amd/csrc/alac_regular.h"
#include "../../saprobe-alac_amd/csrc/alac_plan.h"

extern "C" {

uint32_t plan_sim_keys(void) { return alack::kKeys; }
uint32_t plan_sim_key_wide(void) { return alac::KEY_WIDE; }
uint32_t plan_sim_key_irregular(void) { return alac::KEY_IRREGULAR; }

/* cnt[kKeys] -> the plan's fields; `threads` runs of ceil(kKeys / threads) dispatch positions each (256 on the device).
 * The outputs are pre-filled by the caller: entries the scan does not write keep what they held.
 * totals: nk, total_waves, irr_waves, wide_waves. */
void plan_sim_make(const uint32_t* cnt, uint32_t shift, uint32_t threads, uint32_t* count, uint32_t* pkt_start, uint32_t* list_key,
                   uint32_t* list_wave0, uint32_t* totals) {
    using namespace alack;
    std::vector<Plan> store(1);
    Plan* plan = &store[0];
    memcpy(plan->count, count, sizeof(plan->count));
    memcpy(plan->pkt_start, pkt_start, sizeof(plan->pkt_start));
    memcpy(plan->list_key, list_key, sizeof(plan->list_key));
    memcpy(plan->list_wave0, list_wave0, sizeof(plan->list_wave0));
    const uint32_t run = (kKeys + threads - 1u) / threads;
    std::vector<PlanSums> own(threads);
    for (uint32_t t = 0; t < threads; ++t) own[t] = plan_run_sums(cnt, t * run, run, shift);
    PlanSums front{0u, 0u, 0u, 0u, 0u};
    for (uint32_t t = 0; t < threads; ++t) {
        plan_run_emit(cnt, t * run, run, shift, front, plan);
        front.pkts += own[t].pkts;
        front.waves += own[t].waves;
        front.keys += own[t].keys;
        front.irr += own[t].irr;
        front.wide += own[t].wide;
    }
    plan_totals(front, plan);
    memcpy(count, plan->count, sizeof(plan->count));
    memcpy(pkt_start, plan->pkt_start, sizeof(plan->pkt_start));
    memcpy(list_key, plan->list_key, sizeof(plan->list_key));
    memcpy(list_wave0, plan->list_wave0, sizeof(plan->list_wave0));
    totals[0] = plan->nk;
    totals[1] = plan->total_waves;
    totals[2] = plan->irr_waves;
    totals[3] = plan->wide_waves;
}

} /* extern "C" */
