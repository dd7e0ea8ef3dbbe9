/*
 * k_sort.hip — the sort pre-pass: packet classification + descriptor checks + ranks, the launch plan made by the last block to finish, counting-sort scatter, channel-task keys (one translation unit of libalacgpu.so, see alac_gpu.h).
 */
#include "alac_gpu.h"

namespace alack {

/* ---- what the blocks of a classify kernel do last (the packet sort and the split pipeline's task sort alike) ---------
 * hist: the block's LDS histogram, kKeys words (a task sort fills the first NUM_TASK_KEYS of them, the rest are zero).
 * Every access to the workspace's histogram and ticket is an agent-scope atomic: the blocks of a grid run on all the
 * device's XCDs. */
#define ALAC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

/* One global atomic per key the block saw: it reserves the block's ranks inside the key (a batch has a dozen distinct
 * keys: per-packet global atomics on them serialise). hist[k] turns from the block's count into the block's base rank. */
__device__ __forceinline__ void sort_reserve(uint32_t* hist, uint32_t used, SortWs* ws) {
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < used; k += blockDim.x) {
        const uint32_t c = hist[k];
        if (c) hist[k] = __hip_atomic_fetch_add(&ws->hist[k], c, ALAC_RLX_AGENT);
    }
    __syncthreads();
}

/* The block that finishes last makes the plan; nobody waits for anybody. Each block draws a ticket once its adds to the
 * histogram have come back (sort_reserve: they return a value), and the one that draws the last ticket, and only that
 * one, reads the histogram — complete by then — and writes everything a decode needs of the plan: the counts, the
 * exclusive scan in dispatch order, the totals, and zeros in the gate, balance and queue words of the pair kernels. It
 * then puts the histogram and the ticket back to zero for the next classify kernel on this workspace. All 256 threads of
 * the block take part: each owns a run of consecutive dispatch positions (alac_plan.h), the sums of the runs are scanned
 * with shuffles inside a wave and through LDS across the four waves.
 * No fence on either side of the ticket: the only words one block reads of another's are the histogram's, and those are
 * written by returning atomic adds alone and read by atomic loads, all at agent scope, past every cache that is not shared
 * by the whole device; what a block stores otherwise (keys, ranks, sizes, status) is for the next kernel. A
 * __threadfence() in front of the ticket, which writes each XCD's L2 back once per block, cost the whole gain on the
 * benchmark batch (profiles/r07_presort/). */
__device__ __forceinline__ void sort_finish(uint32_t* hist, SortWs* ws, Plan* plan, uint32_t ppw_shift) {
    __shared__ uint32_t s_last;
    __shared__ uint32_t s_wave[4][5];
    __syncthreads(); /* every thread is done with hist[] (its rank), and the block's adds to the histogram have returned */
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&ws->ticket, 1u, ALAC_RLX_AGENT) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (!s_last) return;
    constexpr uint32_t R = (kKeys + 255u) / 256u;
    {
        /* a thread's R loads are in flight together (one after the other they are R round trips to memory: 33 us for
         * the kernel instead of 9); only the keys that were counted are written back */
        uint32_t c[R];
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t k = threadIdx.x + r * 256u;
            c[r] = k < kKeys ? __hip_atomic_load(&ws->hist[k], ALAC_RLX_AGENT) : 0u;
        }
        if (threadIdx.x == 0) __hip_atomic_store(&ws->ticket, 0u, ALAC_RLX_AGENT);
        uint32_t* z = &plan->gate[0][0]; /* gate, balance and queue lie back to back */
        for (uint32_t k = threadIdx.x; k < kPlanZeroDw; k += 256u) z[k] = 0u;
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
            const uint32_t k = threadIdx.x + r * 256u;
            if (k < kKeys) hist[k] = c[r];
            if (c[r]) __hip_atomic_store(&ws->hist[k], 0u, ALAC_RLX_AGENT);
        }
    }
    __syncthreads();
    const uint32_t q0 = threadIdx.x * R;
    const PlanSums own = plan_run_sums(hist, q0, R, ppw_shift);
    /* inclusive scan over the 64 lanes of the wave */
    uint32_t v[5] = {own.pkts, own.waves, own.keys, own.irr, own.wide};
    const uint32_t lane = threadIdx.x & (kWave - 1u), wave = threadIdx.x / kWave;
#pragma unroll
    for (int o = 1; o < (int)kWave; o <<= 1) {
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint32_t t = (uint32_t)__shfl_up((int)v[j], o, kWave);
            if ((int)lane >= o) v[j] += t;
        }
    }
    if (lane == kWave - 1u)
        for (int j = 0; j < 5; ++j) s_wave[wave][j] = v[j];
    __syncthreads();
    uint32_t all[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        uint32_t front = 0, total = 0;
        for (uint32_t w = 0; w < 4u; ++w) {
            front += w < wave ? s_wave[w][j] : 0u;
            total += s_wave[w][j];
        }
        v[j] += front; /* inclusive over the block */
        all[j] = total;
    }
    plan_run_emit(hist, q0, R, ppw_shift, PlanSums{v[0] - own.pkts, v[1] - own.waves, v[2] - own.keys, v[3] - own.irr, v[4] - own.wide}, plan);
    if (threadIdx.x == 0) plan_totals(PlanSums{all[0], all[1], all[2], all[3], all[4]}, plan);
}
static_assert(offsetof(Plan, queue) + sizeof(Plan::queue) - offsetof(Plan, gate) == kPlanZeroDw * sizeof(uint32_t) &&
                  offsetof(Plan, queue) + sizeof(Plan::queue) == sizeof(Plan),
              "gate, balance and queue are the tail of the plan, back to back");

/* Packet descriptors are checked here, once: a packet must lie inside the blob (the caller's offsets and sizes are
 * untrusted device data). One that does not gets ALACGPU_ERR_RANGE, no sort key, and is never looked at again; the
 * sizes every later kernel uses are the checked copies in sizes_ws. d_sizes may be null: packet i is then
 * blob[offsets[i], offsets[i+1]) (the host entry's offsets[n+1]).
 * The same pass ranks the packet inside its key: the sort-key histogram of the 256-thread block in LDS gives the rank
 * inside the block, sort_reserve the block's base, and rank[i] is stored beside keys[i] for alac_scatter. The last
 * block to finish makes the plan (sort_finish). Launched with 256 threads per block. */
__global__ void __launch_bounds__(256)
alac_classify(alac::DevCfg cfg, const uint8_t* __restrict__ blob, uint64_t blob_bytes, const uint64_t* __restrict__ offsets,
              const uint32_t* __restrict__ sizes, uint32_t n, uint16_t* __restrict__ keys, uint32_t* __restrict__ sizes_ws,
              uint32_t* __restrict__ frames_out, int32_t* __restrict__ status, uint32_t* __restrict__ rank, SortWs* ws, Plan* plan,
              uint32_t ppw_shift) {
    __shared__ uint32_t hist[kKeys];
    for (uint32_t k = threadIdx.x; k < kKeys; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t key = alac::TASK_NONE, local = 0;
    if (i < n) {
        const uint64_t off = offsets[i];
        uint64_t sz = sizes ? (uint64_t)sizes[i] : offsets[i + 1] - off;
        const bool ok = off <= blob_bytes && sz <= blob_bytes - off && sz <= 0x0fffffffull &&
                        (sizes || offsets[i + 1] >= off);
        if (!ok) {
            sizes_ws[i] = 0;
            frames_out[i] = 0;
            status[i] = ALACGPU_ERR_RANGE;
        } else if (sz == 0) {
            /* an empty packet: PastEnd before the first tag (decoder.go:143-145). Settled here so that the readers
             * only ever see packets of at least one byte (their loads are anchored on the packet's last byte). */
            sizes_ws[i] = 0;
            frames_out[i] = 0;
            status[i] = ALACGPU_STATUS(alac::ST_OVERRUN, 0, 0);
        } else {
            sizes_ws[i] = (uint32_t)sz;
            const uint8_t* p = blob + off;
            key = alac::classify_regular(cfg, p, (uint32_t)sz, avail_of(blob_bytes, off));
            /* not regular: scan first (configurations the lean Golomb step covers, alac_regular.h: lean_config). More than two channels: split pipeline. One or two: escape
             * elements are unpacked by alac_interleave, anything else is handed to the whole-packet decoder. */
            if (key == alac::KEY_IRREGULAR) key = alac::lean_config(cfg) ? kKeyScan : kKeyLegacy;
            local = atomicAdd(&hist[key], 1u);
        }
        keys[i] = (uint16_t)key;
    }
    sort_reserve(hist, kKeys, ws);
    if (key != alac::TASK_NONE) rank[i] = hist[key] + local;
    sort_finish(hist, ws, plan, ppw_shift);
}

/* Counting-sort scatter: a packet goes to its key's range of perm[] at the rank alac_classify gave it. The order of
 * packets inside a key is arbitrary (and may differ run to run); results do not depend on it. The threads also zero the
 * claim words behind the plan (claim_dw of them: kClaimDw per wave slot; none behind the split pipeline's plan): nothing
 * reads them before the decode kernels. */
__global__ void __launch_bounds__(256)
alac_scatter(const uint16_t* __restrict__ keys, const uint32_t* __restrict__ rank, uint32_t n, const Plan* __restrict__ plan,
             uint32_t* __restrict__ perm, uint32_t* __restrict__ claims, uint32_t claim_dw) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t k = i; k < claim_dw; k += gridDim.x * blockDim.x) claims[k] = 0u;
    if (i < n) {
        const uint32_t key = keys[i];
        if (key != alac::TASK_NONE) {
            const uint32_t at = plan->pkt_start[key] + rank[i];
            if (at < n) perm[at] = i; /* (always, while the workspace's histogram starts every classify pass from zero) */
        }
    }
}

/* ---- split pipeline (alac_split.h) -------------------------------------------------------------------- */
/* one thread per (packet, bitstream channel): sort key of the channel task, or TASK_NONE; ranks and the plan as in
 * alac_classify */
__global__ void __launch_bounds__(256)
alac_task_classify(alac::DevCfg cfg, const alac::ChanDesc* __restrict__ cd, const alac::PktDesc* __restrict__ pd,
                   const uint16_t* __restrict__ pkt_keys, uint32_t n_slots, uint16_t* __restrict__ keys, uint32_t* __restrict__ rank,
                   SortWs* ws, Plan* plan, uint32_t ppw_shift) {
    __shared__ uint32_t hist[kKeys]; /* the first NUM_TASK_KEYS are this kernel's; all of them the plan's (sort_finish) */
    if (threadIdx.x < alac::NUM_TASK_KEYS) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t key = alac::TASK_NONE, local = 0;
    if (t < n_slots) {
        const uint32_t pkt = t >> 3, slot = t & 7u;
        if (pkt_keys[pkt] == kKeyScan) {
            const alac::PktDesc q = pd[pkt];
            if (q.status == 0 && q.route == alac::ROUTE_SPLIT && slot < q.nslots) {
                const alac::ChanDesc d = cd[t];
                if ((d.info & alac::CD_VALID) && !(d.info & alac::CD_ESCAPE)) key = alac::chan_task_key(cfg, d);
            }
        }
        keys[t] = (uint16_t)key;
        if (key != alac::TASK_NONE) local = atomicAdd(&hist[key], 1u);
    }
    sort_reserve(hist, alac::NUM_TASK_KEYS, ws);
    if (key != alac::TASK_NONE) rank[t] = hist[key] + local;
    sort_finish(hist, ws, plan, ppw_shift);
}
#undef ALAC_RLX_AGENT

/* Which compute units does this device have? Every workgroup marks the one it runs on (same numbering as the pair
 * kernels' gate: XCC_ID << 6 | SE << 4 | CU of HW_ID). 64 KB of LDS each = two workgroups per CU, and the grid is two
 * per CU, so the dispatcher has to use every CU; a workgroup stays until all have arrived (or, on a busy device, for a
 * bounded time: a CU that is missed only loses its fixed place in the pair kernels' item order). Run once per handle. */
__global__ void __launch_bounds__(kWave) alac_cu_census(uint32_t* __restrict__ seen, uint32_t* __restrict__ arrived, uint32_t expect) {
    __shared__ uint32_t pad[16384];
    pad[threadIdx.x] = threadIdx.x;
    if (threadIdx.x == 0) {
        uint32_t id, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        seen[((xcc & 7u) << 6) | (((id >> 13) & 3u) << 4) | ((id >> 8) & 15u)] = 1u;
        atomicAdd(arrived, 1u);
        for (int i = 0; i < 4000 && atomicAdd(arrived, 0u) < expect; ++i) __builtin_amdgcn_s_sleep(32);
    }
    __syncthreads();
    if (pad[(threadIdx.x * 5u) & 63u] == 0xffffffffu) seen[0] = 2u; /* keeps the LDS block allocated */
}

} /* namespace alack */
