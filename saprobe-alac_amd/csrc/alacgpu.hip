/*
 * alacgpu.hip — gfx950 batch ALAC decode kernels + the C ABI of include/alacgpu.h.
 *
 * Replaces the reference's per-packet hot path (decoder.go:133-207 -> internal/alac golomb.go,
 * predictor.go, matrix.go) with HIP kernels over a batch of independent packets. There is no host decode
 * path in this library: every decode entry launches the kernels.
 *
 * One decode = these launches on the handle's stream:
 *   alac_classify  one thread per packet: sort key from the first element header (a few bytes read) and the packet's rank
 *                  inside its key; the last block to finish turns the key histogram into the plan: packet / wave ranges
 *                  (irregular keys, then the longest predictors), the pair kernels' gate words zeroed
 *   alac_scatter   one thread per packet: counting-sort scatter into the lane permutation; zeroes the claim words
 *   alac_scan      irregular packets, one wavefront per 64: status, frame count, where each channel starts; with
 *                  more than two channels also every channel's residuals, into the channel's row
 *   alac_decode_{16,24,32}q   regular packets: entropy, predictor, writer and spare wave per 64 same-key packets
 *                  (alac_duo.h), residuals and samples through an LDS queue; PCM staged in LDS, written in 128-B lines
 *   alac_decode_16l   alac_decode_16q with queue buffers of 32 steps (half as many rendezvous of a workgroup's waves): the
 *                  "fit 4" launch of 16-bit batches that fill the device (long_chunks)
 *   alac_decode_16g, alac_decode_w{24,32}   the gated twin (16-bit batches between the rounds) and the wide keys: a PAIR
 *                  of wavefronts (entropy; predictor + PCM) per 64 same-key packets (one kernel and compilation unit per
 *                  class: sample width x chanBits)
 *   alac_task_classify / alac_scatter / alac_chan_predict   (> 2 channels) one wavefront per 64
 *                  (packet, channel) tasks of the same order: the predictor over the stored residuals, in place
 *   alac_interleave, alac_legacy   PCM of the scanned packets (frame order), whole-packet decoder for the rest
 * alacgpu_waveform_device is a pass of its own behind a decode (k_wave.hip, alac_waveform.h): PCM slots -> planar waveforms.
 * alacgpu_clips_device is another (k_clips.hip, alac_clips.h): PCM slots -> [clips][channels][frames] crops at any frame offset.
 * The kernels live in k_sort.hip, k_scan.hip, k_dec*.hip and k_split.hip (alac_gpu.h).
 * HBM traffic per packet: compressed bytes in, PCM bytes out, plus the U-channel hand-off tile of stereo pairs
 * ((frame_length + 1) x 64 x int32 per workgroup, row-coalesced, written once and read once) or the sample rows
 * of the split pipeline.
 */
#include <cassert>

#include "alac_gpu.h"
#include "alac_host.h"
#include "alac_waveform.h"
#include "alac_clips.h"

using namespace alack;

namespace {
thread_local char g_err[512] = "";
}

void alack::set_err(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

/* ---- host-side copy helpers of the host entry -------------------------------------------------------------- */
namespace {

/* A few worker threads for the staging copies of alacgpu_decode_batch (pageable caller memory <-> pinned staging):
 * one thread moves ~10 GB/s, the PCIe link 50+. Created on first use, joined by alacgpu_destroy. */
class CopyPool {
public:
    explicit CopyPool(unsigned threads) {
        for (unsigned t = 0; t < threads; ++t) workers_.emplace_back([this] { run(); });
    }
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& w : workers_) w.join();
    }
    /* fn(k) for k in [0, tasks), on the workers and on the caller; returns when all are done */
    void parallel_for(size_t tasks, const std::function<void(size_t)>& fn) {
        if (tasks == 0) return;
        if (workers_.empty() || tasks == 1) {
            for (size_t k = 0; k < tasks; ++k) fn(k);
            return;
        }
        {
            std::lock_guard<std::mutex> g(m_);
            fn_ = &fn;
            tasks_ = tasks;
            next_ = 0;
            left_ = tasks;
            ++gen_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return left_ == 0; });
        fn_ = nullptr;
    }

private:
    void work() {
        for (;;) {
            size_t k;
            const std::function<void(size_t)>* fn;
            {
                std::lock_guard<std::mutex> g(m_);
                if (!fn_ || next_ >= tasks_) return;
                k = next_++;
                fn = fn_;
            }
            (*fn)(k);
            std::lock_guard<std::mutex> g(m_);
            if (--left_ == 0) done_.notify_all();
        }
    }
    void run() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m_);
                cv_.wait(l, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            work();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t)>* fn_ = nullptr;
    size_t tasks_ = 0, next_ = 0, left_ = 0;
    uint64_t gen_ = 0;
    bool stop_ = false;
};

/* fn(k) for k in [0, pieces): on the pool if there is one, else on the caller alone */
void copy_pieces(CopyPool* pool, size_t pieces, const std::function<void(size_t)>& fn) {
    if (pool) pool->parallel_for(pieces, fn);
    else for (size_t k = 0; k < pieces; k++) fn(k);
}

constexpr int kSlots = 3; /* chunks in flight in the host entry: one uploading, one decoding, one downloading */

/* one chunk of the host entry: device and pinned staging for its packets and its PCM */
struct Slot {
    DevBuf d_in;   /* [offsets (n+1) x u64 | packet bytes] */
    DevBuf d_out;  /* [PCM n x d_stride | frames n x u32 | status n x i32] */
    HostBuf h_in, h_out;
    hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_out = nullptr;
    size_t first = 0, n = 0;
    bool busy = false;
    bool bad = false; /* the chunk holds descriptors that leave the blob (ALACGPU_ERR_RANGE, set on the way back) */
};

/* Which kernels a handle launches: chosen once per configuration (choose_kernels, called by configure). launch() launches
 * from it and alacgpu_last_dispatch reports from it. Which of the narrow launches WORKS is not in here: that is decode_mode
 * (alac_gpu.h), evaluated on the device and again in alacgpu_last_dispatch. */
struct PairKernel {
    void (*fn)(PairArgs); /* nullptr: the configuration has none */
    const char* name;
};
struct Kernels {
    bool lean;                       /* alac::lean_config: else alac_scan is the whole-packet decoder of every packet */
    bool one_or_two;                 /* channels: with `lean`, the regular packets have kernels of their own; more: the split pipeline */
    PairKernel quad;                 /* narrow regular keys: the four-wave kernel */
    PairKernel quad_long;            /* ... and its form with queue buffers of 32 steps (16-bit only: k_dec16l.hip; long_chunks) */
    PairKernel gated;                /* ... and its gated twin of wave pairs (16-bit only) */
    PairKernel wide;                 /* wide keys: wave pairs (24- and 32-bit only) */
    decltype(&alac_interleave) interleave;
    uint32_t interleave_lds;         /* its dynamic LDS */
    const char* irregular;           /* alacgpu_dispatch::irregular_kernels */
};
#define ALAC_PAIR_KERNEL(k) PairKernel{k, #k}
Kernels choose_kernels(const alac::DevCfg& c) {
    Kernels k{};
    k.lean = alac::lean_config(c); /* pb and kb only: aligned16 has no say */
    k.one_or_two = c.num_channels <= 2;
    k.quad = c.bit_depth == 16 ? ALAC_PAIR_KERNEL(alac_decode_16q) : c.bit_depth == 32 ? ALAC_PAIR_KERNEL(alac_decode_32q) : ALAC_PAIR_KERNEL(alac_decode_24q); /* 24: 20 and 24 */
    k.quad_long = c.bit_depth == 16 ? ALAC_PAIR_KERNEL(alac_decode_16l) : PairKernel{nullptr, ""};
    k.gated = c.bit_depth == 16 ? ALAC_PAIR_KERNEL(alac_decode_16g) : PairKernel{nullptr, ""};
    /* the wide keys (chanBits > 23: 24- and 32-bit streams without their usual shift bytes): wave pairs */
    k.wide = c.bit_depth == 32 ? ALAC_PAIR_KERNEL(alac_decode_w32) : c.bit_depth == 24 ? ALAC_PAIR_KERNEL(alac_decode_w24) : PairKernel{nullptr, ""};
    /* four frames per lane (k_split.hip: alac_interleave4) where the rows exist (more than two channels) and a frame is a whole
     * number of dwords (the layouts with a register-packed form: the others build their frames byte by byte and only lose
     * occupancy to the bigger kernel: 16-bit 3-channel 3.25 -> 3.53 ms) */
    const bool four_frames = c.num_channels > 2 && (c.num_channels * c.bps) % 4u == 0u;
    k.interleave = four_frames ? alac_interleave4 : alac_interleave;
    k.interleave_lds = (four_frames ? 128u : 32u) * kWave;
    k.irregular = !k.lean        ? "alac_scan (whole-packet decoder)"
                  : k.one_or_two ? "alac_scan + alac_interleave (+ alac_legacy)"
                  : four_frames  ? "alac_scan + alac_chan_predict + alac_interleave4 (+ alac_legacy)"
                                 : "alac_scan + alac_chan_predict + alac_interleave (+ alac_legacy)";
    return k;
}
#undef ALAC_PAIR_KERNEL

} /* namespace */

struct alacgpu_decoder {
    alacgpu_config cfg;
    alac::DevCfg dev_cfg;
    Kernels kernels;                                          /* of this configuration */
    int device;
    size_t frame_bytes;
    hipStream_t stream;                                       /* kernels */
    hipStream_t s_in, s_out;                                  /* host entry: uploads, downloads */
    hipStream_t s_side;                                       /* launch(): the irregular packets' kernels beside the regular ones' */
    hipEvent_t ev_fork, ev_join;                              /* s_side leaves `stream` behind the sort and is back before the stop event */
    hipEvent_t ev_start[kTimingSlots], ev_stop[kTimingSlots]; /* ring of per-launch event pairs */
    uint64_t launches;                                       /* since the last timing reset */
    DevBuf scratch_u, scratch_g, plan, cls, perm, sizes_ws;  /* kernel workspace */
    DevBuf rank, sort_ws;                                    /* the sort's ranks (both sorts use them in turn) and its SortWs */
    bool sort_dirty;                                         /* a decode did not get to its end: sort_ws may not be zero */
    DevBuf cd, pd, plan2, keys2, perm2, rows;                /* split pipeline (more than two channels) */
    Slot slots[kSlots];                                      /* host-entry staging */
    CopyPool* pool;
    uint32_t n_cu;                                           /* compute units of the device */
    DevBuf cu_number;                                        /* PairArgs::cu_number */
    size_t chunk_bytes;                                      /* host entry: target bytes (in + out) per chunk */
    uint32_t lanes_min;                                      /* PairArgs::lanes_min; above 16: no second predictor wave for any key */
    int side;                                                /* launch(): irregular packets on s_side (ALACGPU_SIDE: 0 never, 1 up to 6 x CUs wave slots, 2 always: the default) */
    std::thread* ahead;                                      /* alacgpu_decode_batch_start: the decode in flight (nullptr: none) */
    int ahead_rc;
    char ahead_err[512];
    size_t last_n;                                           /* the last device decode: packets, packets per wave slot, PairArgs::cap */
    uint32_t last_ppw, last_cap, last_fit5;
    bool last_long;                                          /* ... and whether its "fit 4" launch was the long-chunk kernel's (long_chunks) */
    bool long_ok;                                            /* ALACGPU_CHUNK=16 (experiments): never */
    uint32_t fit_force;                                      /* PairArgs::fit_force (ALACGPU_FIT) */
    DevBuf wave_ws;                                          /* alacgpu_waveform_device: the scan's scratch */
    hipEvent_t ev_w0, ev_w1;                                 /* around the kernels of the last waveform pass */
    bool wave_timed;
    hipEvent_t ev_c0, ev_c1;                                 /* around the kernels of the last clip gather */
    bool clips_timed;
};

namespace {

size_t plan_claims_offset() { return (sizeof(Plan) + 255u) & ~(size_t)255u; }
size_t plan_bytes(size_t waves) { return plan_claims_offset() + waves * kClaimDw * sizeof(uint32_t); }

/* What launch() asks the runtime about a kernel, asked once per kernel: the cache is keyed by the kernel's address (every
 * pair kernel has the same function type, so a function-local static of a template on that type would be ONE cache for
 * all of them); every device here is the same model.
 * pairs_per_cu: wave pairs of a pair kernel one CU holds at a time (registers and LDS, as the runtime computes it).
 * static_lds: static LDS of a four-wave kernel (what the "fit 4" launch pads up to kQuadLdsFit4: alac_gpu.h). */
struct KernelAttr {
    uint32_t pairs_per_cu, static_lds;
};
KernelAttr kernel_attr(void (*kernel)(PairArgs)) {
    static std::mutex mu;
    static std::vector<std::pair<const void*, KernelAttr>> cache;
    std::lock_guard<std::mutex> g(mu);
    for (const auto& e : cache)
        if (e.first == (const void*)kernel) return e.second;
    int v = 0;
    hipFuncAttributes at;
    KernelAttr a{4u, kQuadLdsFit4}; /* unknown: four pairs; no pad, and no second launch */
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, (int)(2 * kWave), 0) == hipSuccess && v > 0) a.pairs_per_cu = (uint32_t)v;
    else (void)hipGetLastError();
    if (hipFuncGetAttributes(&at, (const void*)kernel) == hipSuccess) a.static_lds = (uint32_t)at.sharedSizeBytes;
    else (void)hipGetLastError();
    cache.emplace_back((const void*)kernel, a);
    return a;
}

/* Numbers the device's compute units for the pair kernels (k_decode_body.inc): XCD by XCD, so that CU number c is on
 * XCD c mod 8 when there are eight of them; within an XCD in the order of the hardware ids. The table is indexed by
 * XCC_ID << 6 | SE << 4 | CU and holds number + 1. */
int cu_numbers(alacgpu_decoder* dec) {
    int rc;
    if ((rc = dec->cu_number.ensure(513 * sizeof(uint32_t)))) return rc;
    HIP_TRY(hipMemsetAsync(dec->cu_number.p, 0, 513 * sizeof(uint32_t), dec->stream));
    hipLaunchKernelGGL(alac_cu_census, dim3(2 * dec->n_cu), dim3(kWave), 0, dec->stream, (uint32_t*)dec->cu_number.p,
                       (uint32_t*)dec->cu_number.p + 512, 2 * dec->n_cu);
    HIP_TRY(hipGetLastError());
    uint32_t seen[512];
    HIP_TRY(hipMemcpyAsync(seen, dec->cu_number.p, sizeof(seen), hipMemcpyDeviceToHost, dec->stream));
    HIP_TRY(hipStreamSynchronize(dec->stream));
    uint32_t per_xcd[8] = {0}, xcds = 0, total = 0;
    for (uint32_t i = 0; i < 512; i++)
        if (seen[i]) {
            per_xcd[i >> 6]++;
            total++;
        }
    for (uint32_t x = 0; x < 8; x++) xcds += per_xcd[x] ? 1u : 0u;
    if (xcds == 0) xcds = 1;
    uint32_t next[8] = {0}, order[8] = {0}, k = 0;
    for (uint32_t x = 0; x < 8; x++)
        if (per_xcd[x]) order[x] = k++;
    for (uint32_t i = 0; i < 512; i++)
        if (seen[i]) {
            const uint32_t x = i >> 6;
            seen[i] = 1u + next[x]++ * xcds + order[x]; /* numbers above n_cu (uneven XCDs) only ever take what is left */
        }
    if (total > dec->n_cu) dec->n_cu = total;
    HIP_TRY(hipMemcpyAsync(dec->cu_number.p, seen, sizeof(seen), hipMemcpyHostToDevice, dec->stream));
    HIP_TRY(hipStreamSynchronize(dec->stream));
    return ALACGPU_E_OK;
}

/* upper bound on the waves of a batch: every key present may end in one partly filled wave. Regular keys: 18 x 18 pairs
 * of predictor orders (0..16 and 31), once more for the wide channels that only 24- and 32-bit streams can have
 * (alac_regular.h: chanBits > 23), plus the irregular keys. */
size_t max_waves(uint32_t bit_depth, size_t n, uint32_t ppw) {
    const size_t keys = (bit_depth >= 24 ? 2 : 1) * 18 * 18 + 8;
    return (n + ppw - 1) / ppw + std::min<size_t>(n, keys);
}
size_t max_waves(const alacgpu_decoder* dec, size_t n, uint32_t ppw) { return max_waves(dec->cfg.bit_depth, n, ppw); }

/* Packets per wave. A VALU instruction costs the SIMD the same whether 64 lanes or 8 are live (profiles/microbench/
 * valu_multi_mi355x.txt, "half" rows), so waves are kept full while there is at least one workgroup per CU (256); a
 * smaller batch is spread over narrower waves to use CUs that would otherwise idle — but no further: a packet is a
 * serial chain whose speed is highest when its wave pair has a CU to itself (4 096 stereo packets: 2.57 ms on 1 024
 * four-lane pairs, 2.19 ms on 256 sixteen-lane pairs; 32 768 packets: 2.63 ms on 1 024 half-full pairs, 2.43 ms on 512
 * full ones). */
uint32_t pick_ppw(size_t n) {
    if (const char* e = getenv("ALACGPU_PPW")) {
        const int v = atoi(e);
        if (v >= 1 && v <= 64 && (v & (v - 1)) == 0) return (uint32_t)v; /* powers of two only */
    }
    uint32_t ppw = kWave;
    while (ppw > 1 && n / ppw < 256) ppw >>= 1;
    return ppw;
}
/* ... always a power of two: the plan's divisions by it are shifts (alac_plan.h) */
uint32_t ppw_shift_of(uint32_t ppw) {
    assert(ppw >= 1u && ppw <= kWave && (ppw & (ppw - 1u)) == 0u);
    return (uint32_t)__builtin_ctz(ppw);
}

size_t row_stride_of(uint32_t frame_length) { return ((size_t)frame_length + 3u) & ~(size_t)3u; } /* 16-byte rows */

int reserve_workspace(alacgpu_decoder* dec, size_t n, uint32_t ppw) {
    const size_t waves = max_waves(dec, n, ppw);
    int rc;
    if ((rc = dec->scratch_u.ensure(waves * u_tile_cells(dec->cfg.frame_length) * sizeof(int32_t)))) return rc;
    if ((rc = dec->scratch_g.ensure(waves * kFallbackSlots * ppw * sizeof(int32_t)))) return rc;
    /* the plan and, behind it, the claim flags of the pair kernels (one per wave slot) */
    if ((rc = dec->plan.ensure(plan_bytes(waves)))) return rc;
    /* the sort's histogram and ticket: zero from here on whenever no classify kernel is running (alac_gpu.h: SortWs) */
    if (!dec->sort_ws.p) {
        if ((rc = dec->sort_ws.ensure(sizeof(SortWs)))) return rc;
        HIP_TRY(hipMemsetAsync(dec->sort_ws.p, 0, sizeof(SortWs), dec->stream));
        dec->sort_dirty = false;
    }
    if ((rc = dec->cls.ensure((n ? n : 1) * sizeof(uint16_t)))) return rc;
    if ((rc = dec->perm.ensure((n ? n : 1) * sizeof(uint32_t)))) return rc;
    if ((rc = dec->sizes_ws.ensure((n ? n : 1) * sizeof(uint32_t)))) return rc;
    const size_t ns = (n ? n : 1) * 8;
    if ((rc = dec->rank.ensure((dec->cfg.num_channels > 2 ? ns : (n ? n : 1)) * sizeof(uint32_t)))) return rc;
    if ((rc = dec->cd.ensure(ns * sizeof(alac::ChanDesc)))) return rc;
    if ((rc = dec->pd.ensure((n ? n : 1) * sizeof(alac::PktDesc)))) return rc;
    if (dec->cfg.num_channels > 2) {
        if ((rc = dec->plan2.ensure(sizeof(Plan)))) return rc;
        if ((rc = dec->keys2.ensure(ns * sizeof(uint16_t)))) return rc;
        if ((rc = dec->perm2.ensure(ns * sizeof(uint32_t)))) return rc;
        if ((rc = dec->rows.ensure((n ? n : 1) * dec->cfg.num_channels * row_stride_of(dec->cfg.frame_length) * sizeof(int32_t))))
            return rc;
    }
    return ALACGPU_E_OK;
}

/* One decode on its way through launch(): the handle, the caller's arguments, and where the irregular packets' kernels go */
struct Launch {
    alacgpu_decoder* dec;
    alac::DevCfg c; /* the handle's, with aligned16 as this call's output allows */
    const uint8_t* d_blob; /* the caller's arguments */
    uint64_t blob_bytes;
    const uint64_t* d_offsets;
    size_t n;
    uint8_t* d_out;
    size_t out_stride;
    uint32_t* d_frames;
    int32_t* d_status;
    uint32_t ppw;
    size_t waves;       /* max_waves of the batch */
    hipStream_t irr;    /* the handle's stream, or s_side when forked */
    bool forked;
    uint32_t scan_grid; /* workgroups of alac_scan / alac_legacy */
    Plan* plan() const { return (Plan*)dec->plan.p; }
    const uint32_t* sz() const { return (const uint32_t*)dec->sizes_ws.p; } /* the checked sizes (alac_classify) */
};

/* s_side beside `stream`: it leaves `stream` behind the sort (ev_fork) and is back before the stop event (ev_join). Between
 * fork() and a join() that got through, an error must not leave s_side running behind the caller's back: whoever drops the
 * fork half-done waits for s_side. */
struct SideFork {
    alacgpu_decoder* dec;
    bool open = false;
    int fork() {
        HIP_TRY(hipEventRecord(dec->ev_fork, dec->stream));
        HIP_TRY(hipStreamWaitEvent(dec->s_side, dec->ev_fork, 0));
        open = true;
        return ALACGPU_E_OK;
    }
    int join() {
        HIP_TRY(hipEventRecord(dec->ev_join, dec->s_side));
        HIP_TRY(hipStreamWaitEvent(dec->stream, dec->ev_join, 0));
        open = false;
        return ALACGPU_E_OK;
    }
    ~SideFork() {
        if (open) (void)hipStreamSynchronize(dec->s_side);
    }
};

/* the sort: keys and ranks, plan, lane permutation — two kernels (k_sort.hip). d_sizes may be null (packet i =
 * blob[offsets[i], offsets[i+1])). The classify kernel counts in the handle's SortWs and leaves it zero again; a decode that
 * failed after it was launched (sort_dirty, cleared by launch() at its end) may not have: zero it first then. */
int sort_pass(const Launch& L, const uint32_t* d_sizes) {
    alacgpu_decoder* dec = L.dec;
    const uint32_t nb = (uint32_t)((L.n + 255) / 256);
    if (dec->sort_dirty) HIP_TRY(hipMemsetAsync(dec->sort_ws.p, 0, sizeof(SortWs), dec->stream));
    dec->sort_dirty = true;
    hipLaunchKernelGGL(alac_classify, dim3(nb), dim3(256), 0, dec->stream, L.c, L.d_blob, L.blob_bytes, L.d_offsets, d_sizes,
                       (uint32_t)L.n, (uint16_t*)dec->cls.p, (uint32_t*)dec->sizes_ws.p, L.d_frames, L.d_status, (uint32_t*)dec->rank.p,
                       (SortWs*)dec->sort_ws.p, L.plan(), ppw_shift_of(L.ppw));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(alac_scatter, dim3(nb), dim3(256), 0, dec->stream, (const uint16_t*)dec->cls.p, (const uint32_t*)dec->rank.p,
                       (uint32_t)L.n, (const Plan*)L.plan(), (uint32_t*)dec->perm.p, (uint32_t*)((uint8_t*)L.plan() + plan_claims_offset()),
                       (uint32_t)(L.waves * kClaimDw));
    return ALACGPU_E_OK;
}

void scan(const Launch& L) {
    alacgpu_decoder* dec = L.dec;
    hipLaunchKernelGGL(alac_scan, dim3(L.scan_grid), dim3(kWave), 0, L.irr, L.c, L.d_blob, L.blob_bytes,
                       L.d_offsets, L.sz(), (const uint32_t*)dec->perm.p, (const Plan*)L.plan(), L.d_out, (uint64_t)L.out_stride, L.d_frames,
                       L.d_status, (int32_t*)dec->scratch_u.p, (int32_t*)dec->scratch_g.p, L.ppw, (alac::ChanDesc*)dec->cd.p,
                       (alac::PktDesc*)dec->pd.p, dec->cfg.num_channels > 2 ? (int32_t*)dec->rows.p : (int32_t*)nullptr,
                       (uint64_t)row_stride_of(dec->cfg.frame_length));
}

/* Whether the "fit 4" launch of a batch of n packets is the long-chunk kernel's (k_dec16l.hip: queue buffers of 32 steps,
 * half as many rendezvous of a workgroup's waves) — decided from what host and device both know, n and ppw, so that
 * alacgpu_last_dispatch can name the kernel that ran. Batches that fill the device: full wave slots, at least one per CU.
 * Below that a workgroup has its CU to itself and the keys with long predictors run predictor waves on several lanes per
 * packet (k_decode_body.inc: lanes_ok, up to n_cu + n_cu / 8 narrow slots), a form the long-chunk unit leaves out; so a
 * batch of that size takes it only where no key would get such waves (lanes_min above 16). Above 4 x CUs slots (`beyond4` in
 * regular_packets) nothing changes: the "fit 5" and the gated launches live on the 26 KB of the short queue, and the rounds of
 * four that such a batch may still run (5 to 7.5 slots per CU, or many irregular packets) stay alac_decode_16q's beside them. */
bool long_chunks(const alacgpu_decoder* dec, size_t n, uint32_t ppw) {
    const size_t slots = (n + ppw - 1) / ppw;
    const uint32_t n_cu = dec->n_cu;
    return dec->kernels.quad_long.fn && dec->long_ok && ppw == kWave && slots >= n_cu && slots <= (size_t)4 * n_cu &&
           (slots > n_cu + n_cu / 8u || dec->lanes_min > 16u);
}

/* one of the up to three launches for the narrow regular wave slots (regular_packets) */
void narrow_launch(const Launch& L, const PairArgs& a, uint32_t slots, uint32_t mode) {
    alacgpu_decoder* dec = L.dec;
    const Kernels& k = dec->kernels;
    if (mode == kModeGated) {
        /* as many workgroups as the device holds at once: they share the slots out among themselves */
        if (a.cap) hipLaunchKernelGGL(k.gated.fn, dim3(std::min<uint32_t>(a.cap * dec->n_cu, slots)), dim3(2 * kWave), 0, dec->stream, a);
        return;
    }
    if (mode == kModeFit5 && !a.fit5) return;
    /* (the long-chunk kernel's static LDS is all but the whole footprint of four per CU: its pad is what is left of it) */
    const PairKernel& pk = (mode == kModeFit4 && dec->last_long) ? k.quad_long : k.quad;
    const uint32_t stat = kernel_attr(pk.fn).static_lds;
    PairArgs q = a;
    q.fit = mode;
    hipLaunchKernelGGL(pk.fn, dim3(slots), dim3(4 * kWave), (mode == kModeFit4 && stat < kQuadLdsFit4) ? kQuadLdsFit4 - stat : 0u,
                       dec->stream, q);
}

/* the regular packets of one or two channels, on the handle's stream */
void regular_packets(const Launch& L) {
    alacgpu_decoder* dec = L.dec;
    const Kernels& k = dec->kernels;
    const size_t n = L.n;
    const uint32_t ppw = L.ppw;
    /* one kernel per class of regular packets (alac_gpu.h, k_decode_body.inc): each one is launched over all the wave
     * slots and leaves the slots of the other classes alone. gated_cap: how many pairs per CU the gated twin of the
     * kernel can hold (0: it has none); which of the twins works is decided on the device. */
    PairArgs a{L.c, L.d_blob, (uint64_t)L.blob_bytes, L.d_offsets, L.sz(), (const uint32_t*)dec->perm.p, L.plan(), L.d_out, (uint64_t)L.out_stride,
               L.d_frames, L.d_status, (int32_t*)dec->scratch_u.p, (const uint32_t*)dec->cu_number.p,
               (uint32_t*)((uint8_t*)L.plan() + plan_claims_offset()), ppw, dec->n_cu, 0u, dec->lanes_min, 4u, dec->fit_force, 0u};
    const uint32_t slots = (uint32_t)L.waves;
    /* The narrow regular wave slots go to ONE of up to three launches, and which one is decided on the device from the
     * plan's count of them (alac_gpu.h: decode_mode; the host only knows an upper bound of ALL slots): the four-wave
     * kernel padded with dynamic LDS to 34 KB per workgroup ("fit 4": four per CU), the same kernel without the pad
     * ("fit 5"), and for 16-bit streams the gated twin of wave pairs. "Fit 4" is always launched; the other two for
     * batches of more than 4 x CUs x 64 packets (`beyond4`), and the device is TOLD whether they are (PairArgs::fit5, cap):
     * it never picks a launch that was not made. (Round 3, found by tools/gpu_fuzz.py: a host-side guess once skipped a
     * launch the device then relied on.) A smaller batch whose many keys push it over 4 x CUs slots all the same runs
     * rounds of four, as in round 3; in exchange the benchmark batch and everything below it see no empty grids at all.
     * The launches that are not the batch's exit at once — but empty grids right IN FRONT of a wave-pair kernel cost it
     * up to 13 % (16-bit 98 304 packets 3.15 -> 3.66 ms with the empty "fit 4" and "fit 5" grids in front of the gated
     * twin, 24-bit stereo without shift bytes 5.2 -> 8.4 ms with both in front of alac_decode_w24; one alone, or any
     * number behind: nothing; the four-wave launches do not care; profiles/r04_final/launch_order*.txt), so the launch
     * the host expects to work — decode_mode() of the batch as if every packet were a narrow regular one — goes first,
     * the wide keys' pairs second, the rest behind. A wrong guess costs speed, never correctness. */
    const uint32_t n_cu = dec->n_cu;
    const bool beyond4 = (n + ppw - 1) / ppw > (size_t)4 * n_cu || dec->fit_force == kModeFit5;
    const bool has_twin = k.gated.fn && beyond4 && dec->fit_force == 0u;
    {
        const uint32_t stat = kernel_attr(k.quad.fn).static_lds;
        a.fit5 = (beyond4 && (size_t)((stat + 1279u) / 1280u) * 1280u * 5u <= 163840u) ? 1u : 0u; /* 1280-byte granules of 160 KB */
    }
    if (has_twin) a.cap = kernel_attr(k.gated.fn).pairs_per_cu;
    if (a.cap <= 4u) a.cap = 0u;
    dec->last_cap = a.cap;
    dec->last_fit5 = a.fit5;
    dec->last_long = long_chunks(dec, n, ppw);
    const uint32_t guess = decode_mode((uint32_t)((n + ppw - 1) / ppw), n_cu, a.cap, dec->fit_force, dec->cfg.num_channels == 1, a.fit5 != 0u);
    narrow_launch(L, a, slots, guess);
    if (k.wide.fn) hipLaunchKernelGGL(k.wide.fn, dim3(slots), dim3(2 * kWave), 0, dec->stream, a);
    for (uint32_t mode : {kModeFit4, kModeFit5, kModeGated})
        if (mode != guess) narrow_launch(L, a, slots, mode);
}

/* more than two channels, behind the scan */
int split_pipeline(const Launch& L) {
    alacgpu_decoder* dec = L.dec;
    /* split pipeline: one lane per channel, sorted by predictor order */
    Plan* plan2 = (Plan*)dec->plan2.p;
    const size_t n_slots = L.n * 8;
    const uint32_t nb2 = (uint32_t)((n_slots + 255) / 256);
    const uint32_t ppw2 = pick_ppw(L.n * dec->cfg.num_channels);
    /* the second sort, in the first one's form and through the same SortWs and ranks (the first sort's kernels are done
     * with both: everything is on the handle's stream); no claim words behind this plan */
    hipLaunchKernelGGL(alac_task_classify, dim3(nb2), dim3(256), 0, dec->stream, L.c, (const alac::ChanDesc*)dec->cd.p,
                       (const alac::PktDesc*)dec->pd.p, (const uint16_t*)dec->cls.p, (uint32_t)n_slots,
                       (uint16_t*)dec->keys2.p, (uint32_t*)dec->rank.p, (SortWs*)dec->sort_ws.p, plan2, ppw_shift_of(ppw2));
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(alac_scatter, dim3(nb2), dim3(256), 0, dec->stream, (const uint16_t*)dec->keys2.p, (const uint32_t*)dec->rank.p,
                       (uint32_t)n_slots, (const Plan*)plan2, (uint32_t*)dec->perm2.p, (uint32_t*)nullptr, 0u);
    hipLaunchKernelGGL(alac_chan_predict, dim3((uint32_t)max_waves(16u, n_slots, ppw2)), dim3(kWave), 0, dec->stream, L.c,
                       L.d_blob, L.blob_bytes, L.d_offsets, L.sz(), (const uint32_t*)dec->perm2.p, (const Plan*)plan2,
                       (const alac::ChanDesc*)dec->cd.p, (int32_t*)dec->rows.p, (uint64_t)row_stride_of(dec->cfg.frame_length), ppw2);
    return ALACGPU_E_OK;
}

/* the irregular packets' PCM: alac_interleave for the scanned ones, alac_legacy (the whole-packet decoder) for the rest */
void irregular_pcm(const Launch& L) {
    alacgpu_decoder* dec = L.dec;
    const Kernels& k = dec->kernels;
    const uint64_t rs = row_stride_of(dec->cfg.frame_length);
    /* slices of a packet (k_split.hip), one wavefront's worth of frames each: one-wave blocks keep more blocks in flight
     * per CU (the kernel waits on memory, not on arithmetic) */
    const uint32_t bpp = (dec->cfg.frame_length + kWave - 1u) / kWave;
    /* PCM of the split packets (with one or two channels: of the escape-only packets) */
    /* a block takes eight slices of a packet at a time (k_split.hip: kSlices) */
    /* (beside the regular packets' kernels: a few blocks per CU — it walks the scanned packets, a handful there) */
    const uint32_t ib = (uint32_t)std::min<uint64_t>((uint64_t)L.n * ((bpp + 7u) / 8u), L.forked ? (uint64_t)4 * dec->n_cu : (uint64_t)32768u);
    hipLaunchKernelGGL(k.interleave, dim3(ib), dim3(kWave), k.interleave_lds, L.irr, L.c, L.d_blob, L.blob_bytes, L.d_offsets, L.sz(),
                       (const uint32_t*)dec->perm.p, (const Plan*)L.plan(), (const alac::ChanDesc*)dec->cd.p,
                       (const alac::PktDesc*)dec->pd.p, (const int32_t*)dec->rows.p, rs, L.d_out, (uint64_t)L.out_stride, bpp);
    hipLaunchKernelGGL(alac_legacy, dim3(L.scan_grid), dim3(kWave), 0, L.irr, L.c, L.d_blob, L.blob_bytes,
                       L.d_offsets, L.sz(), (const uint32_t*)dec->perm.p, (const Plan*)L.plan(), (const alac::PktDesc*)dec->pd.p, L.d_out,
                       (uint64_t)L.out_stride, L.d_frames, L.d_status, (int32_t*)dec->scratch_u.p, (int32_t*)dec->scratch_g.p, L.ppw);
}

/* All kernels of one decode, on the handle's stream. d_sizes may be null (packet i = blob[offsets[i], offsets[i+1])).
 * The event pair brackets everything the decode launches, the sort pre-pass included. */
int launch(alacgpu_decoder* dec, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offsets,
           const uint32_t* d_sizes, size_t n, uint8_t* d_out, size_t out_stride, uint32_t* d_frames, int32_t* d_status) {
    if (n == 0) return ALACGPU_E_OK;
    if (n > 0x7fffffffu) {
        set_err("batch too large");
        return ALACGPU_E_ARG;
    }
    const uint32_t ppw = pick_ppw(n);
    int rc = reserve_workspace(dec, n, ppw);
    if (rc) return rc;
    dec->last_n = n;
    dec->last_ppw = ppw;
    dec->last_cap = dec->last_fit5 = 0;
    dec->last_long = false;
    const Kernels& k = dec->kernels;
    Launch L{dec, dec->dev_cfg, d_blob, blob_bytes, d_offsets, n, d_out, out_stride, d_frames, d_status, ppw, max_waves(dec, n, ppw),
             dec->stream, false, 0u};
    L.c.aligned16 = (out_stride % 16 == 0 && (reinterpret_cast<uintptr_t>(d_out) % 16) == 0) ? 1u : 0u;
    const uint32_t slot = (uint32_t)(dec->launches % kTimingSlots);
    HIP_TRY(hipEventRecord(dec->ev_start[slot], dec->stream));
    if ((rc = sort_pass(L, d_sizes))) return rc;
    /* Packets of one or two channels: what the irregular ones need (alac_scan, then alac_interleave and alac_legacy: a
     * handful of waves, or none) depends on the sort alone and touches no wave slot, packet or descriptor of a regular
     * one, so it runs on a stream of its own BESIDE the workgroups of the regular packets instead of before and behind them
     * (65 536 stereo packets with 328 escape packets among them: 17 + 22 + 4 us and three kernel boundaries off the
     * decode). s_side leaves `stream` behind the sort (ev_fork) and is back before the stop event (ev_join): whoever waits
     * for `stream` waits for it too. With more than two channels the scan IS the decode and everything stays in line.
     * Round 3 did this only for batches of up to 6 x CUs wave slots: alac_scan and alac_legacy were launched with one
     * 201-register, 26-KB workgroup per wave slot of the whole batch and alac_interleave with up to 32 768 blocks, nearly all
     * of which exit at once — but first stand in the dispatcher's line with the later rounds of the decode kernels, on a device
     * whose register files are full (131 072 packets 4.01 -> 4.49 ms). Their grids are bounded now (scan_grid below, k_scan.hip;
     * the interleave grid), and every batch size forks (profiles/r04_final/side_stream.txt: 131 072 packets 3.85 / 3.77 ms in
     * line, 4.00 / 3.76 beside; 196 608: 5.62 -> 5.57; 24-bit 131 072: 4.68 -> 4.65). ALACGPU_SIDE=0: everything in line;
     * 1: round 3's limit of 6 x CUs wave slots. */
    L.forked = k.one_or_two && k.lean &&
               (dec->side >= 2 || (dec->side == 1 && (n + ppw - 1) / ppw <= (size_t)6 * dec->n_cu));
    /* workgroups of alac_scan / alac_legacy: they walk the irregular wave slots (the first plan->irr_waves of the plan,
     * a number only the device knows). Beside the regular packets' kernels: two per CU, a handful of irregular slots is the
     * rule there; where the scan IS the decode (more than two channels, or a configuration the lean kernels do not take):
     * as many as the device holds (201 registers: two waves per SIMD; 26 KB of LDS: six workgroups per CU). */
    L.scan_grid = (uint32_t)std::min<size_t>(L.waves, (size_t)(L.forked ? 2u : 6u) * dec->n_cu);
    /* from here on an error must not leave s_side running behind the caller's back */
    SideFork side{dec};
    if (L.forked) {
        if ((rc = side.fork())) return rc;
        L.irr = dec->s_side;
    }
    /* in line: irregular packets first. Beside: the regular packets' workgroups go first and fill the device (a scan
     * wave needs 201 registers and 26 KB of LDS: it finds room where the first of them have finished, long before the
     * slowest has) */
    if (!L.forked) scan(L);
    if (k.one_or_two && k.lean) regular_packets(L);
    if (L.forked) scan(L);
    HIP_TRY(hipGetLastError());
    if (k.lean) {
        /* irregular packets were only scanned by alac_scan (status, frames, channel descriptors) */
        if (!k.one_or_two && (rc = split_pipeline(L))) return rc;
        irregular_pcm(L);
        HIP_TRY(hipGetLastError());
    }
    if (L.forked && (rc = side.join())) return rc;
    HIP_TRY(hipEventRecord(dec->ev_stop[slot], dec->stream));
    dec->launches++;
    dec->sort_dirty = false; /* every kernel of the decode is in the stream: the classify kernels will run to their end */
    return ALACGPU_E_OK;
}

} /* namespace */

/* ---- handles between uses -------------------------------------------------------------------------------------
 * A file decoder makes a handle, decodes a window or two and destroys it (decode.go:50-80 / stream.py); building one
 * from nothing costs three streams, the events, the CU census with its two synchronisations, and at the first decode a
 * dozen hipMalloc and the pinned staging buffers — 15 ms, where the decode of a 10-second file takes 3. Destroyed
 * handles therefore keep their device-side belongings in a small per-process pool (a few per device, big buffers
 * dropped) and alacgpu_create takes one from there when it can. alacgpu_trim() empties the pool. */
namespace {
std::mutex g_pool_mu;
std::vector<alacgpu_decoder*> g_pool;
std::vector<std::pair<void*, size_t>> g_host_pool;  /* alacgpu_host_free: pinned buffers waiting for the next alacgpu_host_alloc */
std::vector<std::pair<void*, size_t>> g_host_sizes; /* live alacgpu_host_alloc buffers and their sizes */
constexpr size_t kPoolPerDevice = 4;
/* what a pooled handle keeps: device buffers of at most 2 GB in all, pinned host staging of at most 64 MB in all (the
 * largest go first). Device memory is what an MI355X has plenty of (288 GB), and what a file decoder's handles need most of:
 * U hand-off tiles of 1 MB per wave slot, 912 slots for a 1 024-packet window of a 24-bit stream (max_waves) — 1 GB that
 * round 4's first file benchmark allocated and freed per file, with a device-wide hipFree in the middle of the stream.
 * Four handles per device: at most 8 GB of device memory and 0.25 GB of pinned memory per device stay allocated behind
 * alacgpu_destroy() until alacgpu_trim(). */
constexpr size_t kPoolKeepDevice = (size_t)2048 << 20;
constexpr size_t kPoolKeepPinned = (size_t)64 << 20;
/* alacgpu_host_free keeps blocks of up to 64 MB, the eight newest, 192 MB in all (three windows of a file decoder, a few sizes) */
constexpr size_t kHostPoolBlock = (size_t)64 << 20, kHostPoolBytes = (size_t)192 << 20, kHostPoolCount = 8;
template <class Buf>
void keep_at_most(std::vector<Buf*> bufs, size_t limit) {
    for (;;) {
        size_t total = 0;
        Buf* big = nullptr;
        for (Buf* b : bufs) {
            total += b->cap;
            if (b->cap && (!big || b->cap > big->cap)) big = b;
        }
        if (total <= limit || !big) return;
        big->release();
    }
}

/* A handle's belongings, each kind listed ONCE: alacgpu_create makes the streams and events from these lists, alacgpu_destroy
 * trims the buffers of a handle on its way to the pool by them, really_destroy lets go of everything by them. (cu_number is
 * outside the trimming: only really_destroy releases it.) */
std::vector<DevBuf*> device_buffers(alacgpu_decoder* d) {
    std::vector<DevBuf*> v = {&d->scratch_u, &d->scratch_g, &d->plan, &d->cls, &d->perm, &d->sizes_ws, &d->rank, &d->sort_ws, &d->cd, &d->pd,
                              &d->plan2, &d->keys2, &d->perm2, &d->rows, &d->wave_ws};
    for (Slot& s : d->slots) v.insert(v.end(), {&s.d_in, &s.d_out});
    return v;
}
std::vector<HostBuf*> pinned_buffers(alacgpu_decoder* d) {
    std::vector<HostBuf*> v;
    for (Slot& s : d->slots) v.insert(v.end(), {&s.h_in, &s.h_out});
    return v;
}
std::vector<hipStream_t*> streams_of(alacgpu_decoder* d) { return {&d->stream, &d->s_in, &d->s_out, &d->s_side}; }
struct EventRef {
    hipEvent_t* ev;
    unsigned flags;
};
std::vector<EventRef> events_of(alacgpu_decoder* d) {
    std::vector<EventRef> v = {{&d->ev_fork, hipEventDisableTiming}, {&d->ev_join, hipEventDisableTiming},
                               {&d->ev_w0, hipEventDefault}, {&d->ev_w1, hipEventDefault},
                               {&d->ev_c0, hipEventDefault}, {&d->ev_c1, hipEventDefault}};
    for (uint32_t i = 0; i < kTimingSlots; i++) v.insert(v.end(), {{&d->ev_start[i], hipEventDefault}, {&d->ev_stop[i], hipEventDefault}});
    for (Slot& s : d->slots)
        v.insert(v.end(), {{&s.ev_in, hipEventDisableTiming}, {&s.ev_k, hipEventDisableTiming}, {&s.ev_out, hipEventDisableTiming}});
    return v;
}

/* all four streams idle: nothing of this handle's last call is still running */
bool synchronize_all(alacgpu_decoder* d) {
    bool ok = true;
    for (hipStream_t* s : streams_of(d))
        if (*s && hipStreamSynchronize(*s) != hipSuccess) ok = false;
    return ok;
}

void really_destroy(alacgpu_decoder* d) {
    (void)hipSetDevice(d->device);
    (void)synchronize_all(d);
    delete d->pool;
    d->cu_number.release();
    for (DevBuf* b : device_buffers(d)) b->release();
    for (HostBuf* b : pinned_buffers(d)) b->release();
    for (const EventRef& e : events_of(d))
        if (*e.ev) (void)hipEventDestroy(*e.ev);
    for (hipStream_t* s : streams_of(d))
        if (*s) (void)hipStreamDestroy(*s);
    delete d;
}

/* the per-configuration part of a handle (everything else survives in the pool) */
void configure(alacgpu_decoder* d, const alacgpu_config* cfg) {
    const uint32_t bps = alacwf::bytes_per_sample(cfg->bit_depth); /* BytesPerSample, internal/alac/format.go:23-34 */
    d->cfg = *cfg;
    d->frame_bytes = (size_t)cfg->frame_length * cfg->num_channels * (size_t)bps;
    d->dev_cfg = alac::DevCfg{cfg->frame_length, cfg->bit_depth, cfg->num_channels, cfg->pb, cfg->mb, cfg->kb, bps, 0u};
    d->kernels = choose_kernels(d->dev_cfg);
    d->launches = 0;
    d->ahead = nullptr;
    d->ahead_rc = ALACGPU_E_OK;
    d->ahead_err[0] = 0;
    d->last_n = 0;
    d->last_ppw = d->last_cap = d->last_fit5 = 0;
    d->last_long = false;
    d->wave_timed = false;
    d->clips_timed = false;
    d->lanes_min = 4;
    d->fit_force = 0;
    if (const char* e = getenv("ALACGPU_FIT")) d->fit_force = (uint32_t)atoi(e); /* experiments: 4 / 5 workgroups per CU for every batch */
    if (const char* e = getenv("ALACGPU_LANES_MIN")) d->lanes_min = (uint32_t)std::max(1, atoi(e)); /* experiments; 17: never */
    d->long_ok = true;
    if (const char* e = getenv("ALACGPU_CHUNK")) d->long_ok = atoi(e) != 16; /* experiments (A/B): 16 keeps every batch on alac_decode_16q */
    d->side = 2;
    if (const char* e = getenv("ALACGPU_SIDE")) d->side = atoi(e); /* experiments, tests */
    d->chunk_bytes = (size_t)192 << 20;
    if (const char* e = getenv("ALACGPU_CHUNK_MB")) {
        const long v = atol(e);
        if (v >= 1 && v <= 65536) d->chunk_bytes = (size_t)v << 20;
    }
}
} /* namespace */

static int settle_ahead(alacgpu_decoder* d);

/* what the two decode entries ask of their arguments alike */
static int check_decode_args(const alacgpu_decoder* d, const void* blob, size_t blob_bytes, const void* offsets, size_t n, const void* out,
                             size_t out_stride, const void* frames, const void* status) {
    if (!d || (n && (!offsets || !out || !frames || !status)) || (blob_bytes && !blob)) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    if (out_stride < d->frame_bytes) {
        set_err("out_stride %zu < frame bytes %zu", out_stride, d->frame_bytes);
        return ALACGPU_E_ARG;
    }
    return ALACGPU_E_OK;
}

extern "C" {

int alacgpu_create(const alacgpu_config* cfg, int device, alacgpu_decoder** out) {
    if (!cfg || !out) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    *out = nullptr;
    if (int rc = check_config(cfg)) return rc;
    HIP_TRY(hipSetDevice(device));
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = 0; i < g_pool.size(); i++)
            if (g_pool[i]->device == device) {
                alacgpu_decoder* d = g_pool[i];
                g_pool.erase(g_pool.begin() + (long)i);
                configure(d, cfg);
                *out = d;
                return ALACGPU_E_OK;
            }
    }
    alacgpu_decoder* d = new (std::nothrow) alacgpu_decoder();
    if (!d) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    d->device = device; /* (value-initialised: every stream, event and buffer of the new handle is null) */
    configure(d, cfg);
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
        d->n_cu = cus > 0 ? (uint32_t)cus : 256u;
    }
    hipError_t e = hipSuccess;
    /* (the default priority: at the lowest one the side kernels linger until the decode's last workgroups have gone and
     * become its tail: 131 072 packets 3.85 -> 4.38 ms, 24-bit 4.68 -> 5.97; profiles/r04_final/side_stream.txt) */
    for (hipStream_t* st : streams_of(d))
        if (e == hipSuccess) e = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    for (const EventRef& ev : events_of(d))
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev.ev, ev.flags);
    if (e != hipSuccess) {
        set_err("stream/event creation failed: %s", hipGetErrorString(e));
        really_destroy(d);
        return ALACGPU_E_HIP;
    }
    if (int rc = cu_numbers(d)) {
        really_destroy(d);
        return rc;
    }
    *out = d;
    return ALACGPU_E_OK;
}

void alacgpu_destroy(alacgpu_decoder* d) {
    if (!d) return;
    (void)settle_ahead(d);
    (void)hipSetDevice(d->device);
    /* nothing of this handle's last call may still be running when its belongings go to the next owner */
    if (synchronize_all(d)) {
        for (int k = 0; k < kSlots; k++) d->slots[k].busy = false;
        if (d->sort_dirty) d->sort_ws.release(); /* a handle comes back from the pool clean: allocated again and zeroed by its next decode */
        d->sort_dirty = false;
        keep_at_most(device_buffers(d), kPoolKeepDevice);
        keep_at_most(pinned_buffers(d), kPoolKeepPinned);
        std::lock_guard<std::mutex> g(g_pool_mu);
        size_t same = 0;
        for (alacgpu_decoder* p : g_pool) same += p->device == d->device ? 1u : 0u;
        if (same < kPoolPerDevice) {
            g_pool.push_back(d);
            return;
        }
    }
    really_destroy(d);
}

void alacgpu_trim(void) {
    std::vector<alacgpu_decoder*> all;
    std::vector<std::pair<void*, size_t>> host;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        all.swap(g_pool);
        host.swap(g_host_pool);
    }
    for (alacgpu_decoder* d : all) really_destroy(d);
    for (auto& h : host) (void)hipHostFree(h.first);
}

/* Pinned host memory for a caller's PCM (or packet) buffers: what alacgpu_decode_batch finds in pinned memory it
 * transfers in place, without the copy through its staging. Freed buffers of up to 64 MB are kept (the eight newest, 192 MB
 * in all; the smallest that fits is handed out again): a file decoder asks for the same sizes file after file, and
 * hipHostMalloc / hipHostFree cost milliseconds each and stall the device. */
void* alacgpu_host_alloc(size_t bytes) {
    if (bytes == 0) bytes = 1;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        size_t best = SIZE_MAX;
        for (size_t i = 0; i < g_host_pool.size(); i++)
            if (g_host_pool[i].second >= bytes && g_host_pool[i].second <= 2 * bytes + (1u << 20) &&
                (best == SIZE_MAX || g_host_pool[i].second < g_host_pool[best].second))
                best = i;
        if (best != SIZE_MAX) {
            void* p = g_host_pool[best].first;
            g_host_sizes.emplace_back(p, g_host_pool[best].second);
            g_host_pool.erase(g_host_pool.begin() + (long)best);
            return p;
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        set_err("hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    std::lock_guard<std::mutex> g(g_pool_mu);
    g_host_sizes.emplace_back(p, bytes);
    return p;
}

void alacgpu_host_free(void* p) {
    if (!p) return;
    size_t bytes = 0;
    std::vector<void*> evict;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = 0; i < g_host_sizes.size(); i++)
            if (g_host_sizes[i].first == p) {
                bytes = g_host_sizes[i].second;
                g_host_sizes.erase(g_host_sizes.begin() + (long)i);
                break;
            }
        if (bytes && bytes <= kHostPoolBlock) {
            /* newest last; what no longer fits goes oldest first (round 4: a pool of four blocks, first come first kept,
             * filled up with the small windows of short files and then made every long file allocate and free its own) */
            g_host_pool.emplace_back(p, bytes);
            p = nullptr;
            size_t total = 0;
            for (const auto& h : g_host_pool) total += h.second;
            while (g_host_pool.size() > kHostPoolCount || total > kHostPoolBytes) {
                evict.push_back(g_host_pool.front().first);
                total -= g_host_pool.front().second;
                g_host_pool.erase(g_host_pool.begin());
            }
        }
    }
    for (void* q : evict) (void)hipHostFree(q);
    if (p) (void)hipHostFree(p);
}

int alacgpu_get_format(const alacgpu_decoder* d, alacgpu_format* fmt) {
    if (!d || !fmt) return ALACGPU_E_ARG;
    fmt->sample_rate = (int32_t)d->cfg.sample_rate; /* decoder.go:98-102 */
    fmt->bit_depth = d->cfg.bit_depth;
    fmt->channels = d->cfg.num_channels;
    return ALACGPU_E_OK;
}

size_t alacgpu_frame_bytes(const alacgpu_decoder* d) { return d ? d->frame_bytes : 0; }

int alacgpu_reserve(alacgpu_decoder* d, size_t n) {
    if (!d) return ALACGPU_E_ARG;
    HIP_TRY(hipSetDevice(d->device));
    if (int rc = d->wave_ws.ensure(alack::wave_scratch_bytes(n))) return rc;
    return reserve_workspace(d, n, pick_ppw(n));
}

/* the decode alacgpu_decode_batch_start put on a thread of its own, if any: wait for it and take over its result */
static int settle_ahead(alacgpu_decoder* d) {
    if (!d->ahead) return ALACGPU_E_OK;
    d->ahead->join();
    delete d->ahead;
    d->ahead = nullptr;
    if (d->ahead_rc != ALACGPU_E_OK) set_err("%s", d->ahead_err);
    return d->ahead_rc;
}

int alacgpu_decode_batch_start(alacgpu_decoder* d, const uint8_t* blob, size_t blob_bytes, const uint64_t* offsets, size_t n,
                               uint8_t* out, size_t out_stride, uint32_t* frames_out, int32_t* status) {
    if (!d) return ALACGPU_E_ARG;
    if (d->ahead) {
        set_err("a decode started with alacgpu_decode_batch_start is still in flight: alacgpu_decode_batch_wait first");
        return ALACGPU_E_ARG;
    }
    d->ahead_rc = ALACGPU_E_OK;
    d->ahead = new (std::nothrow) std::thread([=] {
        d->ahead_rc = alacgpu_decode_batch(d, blob, blob_bytes, offsets, n, out, out_stride, frames_out, status);
        if (d->ahead_rc != ALACGPU_E_OK) snprintf(d->ahead_err, sizeof(d->ahead_err), "%s", alacgpu_last_error());
    });
    if (!d->ahead) {
        set_err("out of memory");
        return ALACGPU_E_ARG;
    }
    return ALACGPU_E_OK;
}

int alacgpu_decode_batch_wait(alacgpu_decoder* d) {
    if (!d) return ALACGPU_E_ARG;
    return settle_ahead(d);
}

int alacgpu_decode_batch_device(alacgpu_decoder* d, const uint8_t* d_blob, size_t blob_bytes, const uint64_t* d_offsets,
                                const uint32_t* d_sizes, size_t n, uint8_t* d_out, size_t out_stride,
                                uint32_t* d_frames, int32_t* d_status, int sync) {
    int rc = check_decode_args(d, d_blob, blob_bytes, d_offsets, n, d_out, out_stride, d_frames, d_status);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(d->device));
    rc = launch(d, d_blob, (uint64_t)blob_bytes, d_offsets, d_sizes, n, d_out, out_stride, d_frames, d_status);
    if (rc) return rc;
    if (sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return ALACGPU_E_OK;
}

/*
 * DecodePackets from host memory: the batch is cut into chunks of whole packets; chunk c is uploaded on one stream
 * while chunk c-1 decodes on the handle's stream and chunk c-2 comes back on a third. The packets go up exactly as
 * they lie in the caller's blob (no re-pack: the kernels read dense blobs), together with their offsets and sizes, in
 * ONE transfer; PCM, frame counts and status words come back in ONE. Pageable caller memory is staged through pinned
 * buffers by a few copy threads; memory the caller pinned itself (hipHostMalloc / hipHostRegister) is used in place.
 * The offsets are untrusted (a sample table read from a file): a packet that does not lie inside [0, blob_bytes), or
 * whose end lies before its start, is never read; it gets ALACGPU_ERR_RANGE like in the device entry.
 */
int alacgpu_decode_batch(alacgpu_decoder* d, const uint8_t* blob, size_t blob_bytes, const uint64_t* offsets, size_t n,
                         uint8_t* out, size_t out_stride, uint32_t* frames_out, int32_t* status) {
    if (int rc = check_decode_args(d, blob, blob_bytes, offsets, n, out, out_stride, frames_out, status)) return rc;
    if (n == 0) return ALACGPU_E_OK;
    auto valid = [&](size_t i) {
        const uint64_t lo = offsets[i], hi = offsets[i + 1];
        return lo <= hi && hi <= (uint64_t)blob_bytes && hi - lo <= 0x0fffffffull;
    };
    HIP_TRY(hipSetDevice(d->device));
    const size_t fb = d->frame_bytes;
    const size_t d_stride = (fb + 15u) & ~(size_t)15u; /* 16-byte aligned device rows: the LDS-staged wide stores */
    const bool out_pinned = is_pinned(out) && is_pinned(frames_out) && is_pinned(status);
    const bool in_pinned = blob_bytes == 0 || is_pinned(blob);
    if (!d->pool && !(out_pinned && in_pinned)) {
        unsigned t = std::thread::hardware_concurrency();
        t = t > 16 ? 8 : (t > 2 ? t / 2 : 1);
        if (const char* e = getenv("ALACGPU_COPY_THREADS")) t = (unsigned)std::max(1, atoi(e));
        d->pool = new (std::nothrow) CopyPool(t - 1); /* the calling thread copies too */
    }

    /* chunk is back in pinned memory (or in place): hand it to the caller; descriptors that left the blob get their
     * status here (the device saw them as empty packets) */
    auto finish = [&](Slot& s) -> int {
        HIP_TRY(hipEventSynchronize(s.ev_out));
        if (!out_pinned) {
            const uint8_t* h = (const uint8_t*)s.h_out.p;
            const uint8_t* hm = h + s.n * d_stride;
            memcpy(frames_out + s.first, hm, s.n * sizeof(uint32_t));
            memcpy(status + s.first, hm + s.n * sizeof(uint32_t), s.n * sizeof(int32_t));
            const size_t pieces = std::min<size_t>(s.n, 64);
            auto body = [&](size_t k) {
                const size_t lo = s.n * k / pieces, hi = s.n * (k + 1) / pieces;
                /* one copy per piece only where the rows have no gap: the staging's bytes [fb, d_stride) are stale, and the
                 * caller's [fb, out_stride) is the caller's (a 16-byte stride over frames of fb % 16 != 0 bytes) */
                if (out_stride == fb && d_stride == fb) {
                    memcpy(out + (s.first + lo) * out_stride, h + lo * d_stride, (hi - lo) * fb);
                } else {
                    for (size_t i = lo; i < hi; i++) memcpy(out + (s.first + i) * out_stride, h + i * d_stride, fb);
                }
            };
            copy_pieces(d->pool, pieces, body);
        }
        if (s.bad)
            for (size_t i = s.first; i < s.first + s.n; i++)
                if (!valid(i)) {
                    status[i] = ALACGPU_ERR_RANGE;
                    frames_out[i] = 0;
                }
        /* The kernels leave the bytes behind a partial frame alone, and the device-side PCM slots of a (pooled) handle
         * hold whatever an earlier batch left there: the caller gets zeros instead, as from DecodePacket's zeroed frame
         * buffer (decoder.go:120,127). One packet in a hundred has a partial frame. */
        {
            const size_t bpf = fb / d->cfg.frame_length; /* bytes per frame */
            for (size_t i = s.first; i < s.first + s.n; i++) {
                const size_t have = std::min<size_t>(frames_out[i], d->cfg.frame_length) * bpf;
                if (have < fb) memset(out + i * out_stride + have, 0, fb - have);
            }
        }
        s.busy = false;
        return ALACGPU_E_OK;
    };
    /* one chunk: upload, decode, download, all asynchronous; HIP errors come back as a code so that the caller drains */
    auto submit = [&](Slot& s, size_t first, size_t cnt, uint64_t lo, uint64_t hi) -> int {
        int rc;
        s.first = first;
        s.n = cnt;
        s.bad = false;
        const size_t in_bytes = (size_t)(hi - lo);
        const size_t meta = (cnt + 1) * sizeof(uint64_t) + cnt * sizeof(uint32_t);
        const size_t meta_pad = (meta + 255u) & ~(size_t)255u; /* packet bytes start 256-byte aligned on the device */
        if ((rc = s.d_in.ensure(meta_pad + in_bytes + 16))) return rc;
        if ((rc = s.d_out.ensure(cnt * d_stride + cnt * 8 + 16))) return rc;
        if ((rc = s.h_in.ensure(in_pinned ? meta_pad : meta_pad + in_bytes))) return rc;
        if (!out_pinned && (rc = s.h_out.ensure(cnt * d_stride + cnt * 8))) return rc;
        /* upload: offsets rebased to the chunk's first byte and sizes, then the bytes */
        uint64_t* h_off = (uint64_t*)s.h_in.p;
        uint32_t* h_sz = (uint32_t*)(h_off + cnt + 1);
        for (size_t i = 0; i < cnt; i++) {
            const bool ok = valid(first + i);
            h_off[i] = ok ? offsets[first + i] - lo : 0u;
            h_sz[i] = ok ? (uint32_t)(offsets[first + i + 1] - offsets[first + i]) : 0u;
            s.bad = s.bad || !ok;
        }
        h_off[cnt] = in_bytes;
        uint8_t* d_in = (uint8_t*)s.d_in.p;
        if (in_pinned) {
            HIP_TRY(hipMemcpyAsync(d_in, h_off, meta, hipMemcpyHostToDevice, d->s_in));
            if (in_bytes) HIP_TRY(hipMemcpyAsync(d_in + meta_pad, blob + lo, in_bytes, hipMemcpyHostToDevice, d->s_in));
        } else {
            uint8_t* hb = (uint8_t*)s.h_in.p + meta_pad;
            const size_t pieces = std::max<size_t>(1, std::min<size_t>(64, in_bytes >> 20));
            auto body = [&](size_t k) {
                const size_t a = in_bytes * k / pieces, b = in_bytes * (k + 1) / pieces;
                memcpy(hb + a, blob + lo + a, b - a);
            };
            copy_pieces(d->pool, pieces, body);
            HIP_TRY(hipMemcpyAsync(d_in, s.h_in.p, meta_pad + in_bytes, hipMemcpyHostToDevice, d->s_in));
        }
        HIP_TRY(hipEventRecord(s.ev_in, d->s_in));
        /* decode */
        HIP_TRY(hipStreamWaitEvent(d->stream, s.ev_in, 0));
        uint8_t* d_pcm = (uint8_t*)s.d_out.p;
        uint32_t* d_fr = (uint32_t*)(d_pcm + cnt * d_stride);
        int32_t* d_st = (int32_t*)(d_fr + cnt);
        if ((rc = launch(d, d_in + meta_pad, in_bytes, (const uint64_t*)d_in, (const uint32_t*)(d_in + (cnt + 1) * sizeof(uint64_t)), cnt,
                         d_pcm, d_stride, d_fr, d_st)))
            return rc;
        HIP_TRY(hipEventRecord(s.ev_k, d->stream));
        /* download */
        HIP_TRY(hipStreamWaitEvent(d->s_out, s.ev_k, 0));
        if (out_pinned) {
            HIP_TRY(hipMemcpy2DAsync(out + first * out_stride, out_stride, d_pcm, d_stride, fb, cnt, hipMemcpyDeviceToHost, d->s_out));
            HIP_TRY(hipMemcpyAsync(frames_out + first, d_fr, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, d->s_out));
            HIP_TRY(hipMemcpyAsync(status + first, d_st, cnt * sizeof(int32_t), hipMemcpyDeviceToHost, d->s_out));
        } else {
            HIP_TRY(hipMemcpyAsync(s.h_out.p, d_pcm, cnt * d_stride + cnt * 8, hipMemcpyDeviceToHost, d->s_out));
        }
        HIP_TRY(hipEventRecord(s.ev_out, d->s_out));
        s.busy = true;
        return ALACGPU_E_OK;
    };

    size_t first = 0;
    int turn = 0;
    int rc = ALACGPU_E_OK;
    while (first < n && rc == ALACGPU_E_OK) {
        /* packets of this chunk: whole packets, about chunk_bytes of traffic (the span of the blob they cover in + PCM
         * out). With a sane table the span is offsets[first] .. offsets[first + cnt]. */
        size_t cnt = 0;
        uint64_t lo = ~0ull, hi = 0;
        while (first + cnt < n) {
            uint64_t nlo = lo, nhi = hi;
            if (valid(first + cnt)) {
                nlo = std::min(lo, offsets[first + cnt]);
                nhi = std::max(hi, offsets[first + cnt + 1]);
            }
            const uint64_t bytes = (nhi > nlo ? nhi - nlo : 0) + (uint64_t)(cnt + 1) * fb;
            if (cnt != 0 && bytes > d->chunk_bytes) break;
            lo = nlo;
            hi = nhi;
            cnt++;
        }
        if (hi < lo) lo = hi = 0; /* no valid packet in the chunk */
        Slot& s = d->slots[turn];
        turn = (turn + 1) % kSlots;
        if (s.busy && (rc = finish(s))) break;
        rc = submit(s, first, cnt, lo, hi);
        first += cnt;
    }
    if (rc != ALACGPU_E_OK) {
        /* a step of a chunk failed: nothing of this call may still be writing the caller's buffers when we return, and
         * no slot may carry a chunk of this call into the next one */
        (void)hipStreamSynchronize(d->s_in);
        (void)hipStreamSynchronize(d->stream);
        (void)hipStreamSynchronize(d->s_side);
        (void)hipStreamSynchronize(d->s_out);
        for (int k = 0; k < kSlots; k++) d->slots[k].busy = false;
        return rc;
    }
    /* drain, oldest first */
    for (int k = 0; k < kSlots; k++) {
        Slot& s = d->slots[(turn + k) % kSlots];
        if (!s.busy) continue;
        const int r2 = finish(s);
        if (rc == ALACGPU_E_OK) rc = r2;
        s.busy = false;
    }
    return rc;
}

int alacgpu_decode_packet(alacgpu_decoder* d, const uint8_t* packet, size_t packet_len, uint8_t* out, size_t out_cap,
                          size_t* out_len, int32_t* status_out) {
    if (!d || (!packet && packet_len) || !out || !out_len) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    if (out_cap < d->frame_bytes) { /* decodePacketInto needs a full frame, decoder.go:131-132 */
        set_err("output capacity %zu < frame bytes %zu", out_cap, d->frame_bytes);
        return ALACGPU_E_ARG;
    }
    *out_len = 0;
    const uint64_t offs[2] = {0, packet_len};
    const uint8_t dummy = 0;
    uint32_t frames = 0;
    int32_t st = 0;
    /* a batch of one through the same entry: one upload (offsets + bytes), the kernels, one download */
    int rc = alacgpu_decode_batch(d, packet_len ? packet : &dummy, packet_len, offs, 1, out, d->frame_bytes, &frames, &st);
    if (rc) return rc;
    if (status_out) *status_out = st;
    if (st != 0) {
        set_err("decode failed: status 0x%x", st);
        return ALACGPU_E_DECODE;
    }
    *out_len = (size_t)frames * d->cfg.num_channels * (size_t)d->dev_cfg.bps; /* decoder.go:206 */
    return ALACGPU_E_OK;
}

int alacgpu_timing_reset(alacgpu_decoder* d) {
    if (!d) return ALACGPU_E_ARG;
    d->launches = 0;
    return ALACGPU_E_OK;
}

int alacgpu_kernel_times(alacgpu_decoder* d, float* ms, size_t max_n, size_t* n_out) {
    if (!d || !ms || !n_out) return ALACGPU_E_ARG;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    size_t avail = (size_t)std::min<uint64_t>(d->launches, kTimingSlots);
    size_t n = std::min(avail, max_n);
    /* the n most recent launches, oldest first */
    for (size_t i = 0; i < n; i++) {
        const uint32_t slot = (uint32_t)((d->launches - n + i) % kTimingSlots);
        HIP_TRY(hipEventElapsedTime(&ms[i], d->ev_start[slot], d->ev_stop[slot]));
    }
    *n_out = n;
    return ALACGPU_E_OK;
}

int alacgpu_pair_placement(alacgpu_decoder* d, uint32_t* tags, size_t max_n, size_t* n_out) {
    if (!d || !tags || !n_out) return ALACGPU_E_ARG;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    *n_out = 0;
    if (!d->plan.p) return ALACGPU_E_OK;
    Plan head;
    HIP_TRY(hipMemcpy(&head, d->plan.p, sizeof(Plan), hipMemcpyDeviceToHost));
    const size_t n = std::min<size_t>(head.total_waves, max_n / kClaimDw);
    if (plan_bytes(n) > d->plan.cap) return ALACGPU_E_ARG;
    if (n) HIP_TRY(hipMemcpy(tags, (const uint8_t*)d->plan.p + plan_claims_offset(), n * kClaimDw * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n_out = n;
    return ALACGPU_E_OK;
}

int alacgpu_last_dispatch(alacgpu_decoder* d, alacgpu_dispatch* out) {
    if (!d || !out) return ALACGPU_E_ARG;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    memset(out, 0, sizeof(*out));
    if (!d->plan.p || d->last_n == 0) return ALACGPU_E_OK;
    Plan head;
    HIP_TRY(hipMemcpy(&head, d->plan.p, sizeof(Plan), hipMemcpyDeviceToHost));
    out->packets_per_slot = d->last_ppw;
    out->slots = head.total_waves;
    out->irregular_slots = head.irr_waves;
    out->wide_slots = head.wide_waves;
    out->narrow_slots = head.total_waves - head.irr_waves - head.wide_waves;
    out->keys = head.nk;
    const Kernels& k = d->kernels;
    const bool lean = k.one_or_two && k.lean;
    /* the device's own decision (k_decode_body.inc reads the same plan and calls the same function) */
    const char* narrow = "";
    if (lean && out->narrow_slots) {
        const uint32_t mode = decode_mode(out->narrow_slots, d->n_cu, d->last_cap, d->fit_force, d->cfg.num_channels == 1, d->last_fit5 != 0u);
        const bool lng = mode == kModeFit4 && d->last_long;
        narrow = mode == kModeGated ? k.gated.name : lng ? k.quad_long.name : k.quad.name;
        out->gated = mode == kModeGated ? 1u : 0u;
        out->workgroups_per_cu = mode == kModeGated ? pair_quota(out->narrow_slots, d->n_cu, d->last_cap) : mode;
        /* predictor waves on several lanes per packet (k_decode_body.inc: lanes_ok) */
        if (!out->gated && !lng && out->narrow_slots <= d->n_cu + d->n_cu / 8u && d->lanes_min <= 16u) out->lanes_per_packet = d->last_ppw <= 32u ? 4u : 2u;
    }
    snprintf(out->narrow_kernel, sizeof(out->narrow_kernel), "%s", narrow);
    snprintf(out->wide_kernel, sizeof(out->wide_kernel), "%s", (lean && out->wide_slots) ? k.wide.name : "");
    snprintf(out->irregular_kernels, sizeof(out->irregular_kernels), "%s", out->irregular_slots ? k.irregular : "");
    return ALACGPU_E_OK;
}

int alacgpu_last_kernel_ms(alacgpu_decoder* d, float* ms) {
    size_t got = 0;
    int rc = alacgpu_kernel_times(d, ms, 1, &got);
    if (rc) return rc;
    if (got == 0) {
        set_err("no kernel has been launched on this handle since the last timing reset");
        return ALACGPU_E_ARG;
    }
    return ALACGPU_E_OK;
}

int alacgpu_waveform_device(alacgpu_decoder* d, const uint8_t* d_pcm, size_t pcm_stride, const uint32_t* d_frames,
                            const int32_t* d_status, size_t n, int layout, int type, void* d_wave, size_t channel_stride,
                            size_t packet_stride, uint64_t* d_starts, int sync) {
    if (!d || (n && (!d_pcm || !d_frames || !d_wave))) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    if ((layout != ALACGPU_WAVE_STREAM && layout != ALACGPU_WAVE_PACKETS) || (type != ALACGPU_WAVE_FLOAT && type != ALACGPU_WAVE_INT)) {
        set_err("unknown waveform layout %d or type %d", layout, type);
        return ALACGPU_E_ARG;
    }
    if (n > 0x7fffffffu) {
        set_err("batch too large");
        return ALACGPU_E_ARG;
    }
    const uint64_t fl = d->cfg.frame_length, ch = d->cfg.num_channels;
    if (n) {
        if (pcm_stride < d->frame_bytes) {
            set_err("pcm_stride %zu < frame bytes %zu", pcm_stride, d->frame_bytes);
            return ALACGPU_E_ARG;
        }
        if (reinterpret_cast<uintptr_t>(d_wave) % 4) {
            set_err("d_wave is not aligned to its 4-byte elements");
            return ALACGPU_E_ARG;
        }
        /* with f[i] <= frame_length (the kernels clamp) these bounds keep every column inside its row whatever d_frames holds */
        if (layout == ALACGPU_WAVE_STREAM ? channel_stride < (uint64_t)n * fl
                                          : (channel_stride < fl || packet_stride / ch < channel_stride)) {
            set_err("channel_stride %zu / packet_stride %zu too small for %zu packets of %u frames", channel_stride, packet_stride, n,
                    d->cfg.frame_length);
            return ALACGPU_E_ARG;
        }
    }
    HIP_TRY(hipSetDevice(d->device));
    /* Growing the scratch frees it first, while an earlier pass with sync = 0 and a smaller n may still be queued on the
     * stream and reading it: that is safe only because hipFree waits for the whole device before it lets go of the memory
     * (the same holds for the decode's workspace, alacgpu_reserve's comment in alacgpu.h). Callers that queue passes back
     * to back reserve for their largest batch first and never get here with a buffer to grow. */
    if (n && (layout == ALACGPU_WAVE_STREAM || d_starts)) {
        if (int rc = d->wave_ws.ensure(alack::wave_scratch_bytes(n))) return rc;
    }
    alacwf::Params p = alacwf::make_params(d->cfg.frame_length, d->cfg.bit_depth, d->cfg.num_channels, (uint32_t)layout, (uint32_t)type);
    p.pcm = d_pcm;
    p.pcm_stride = pcm_stride;
    p.frames = d_frames;
    p.status = d_status;
    p.wave = (uint8_t*)d_wave;
    p.channel_stride = channel_stride;
    p.packet_stride = packet_stride;
    p.n = n;
    HIP_TRY(hipEventRecord(d->ev_w0, d->stream));
    HIP_TRY(alack::wave_launch(d->stream, p, d_starts, d->wave_ws.p));
    HIP_TRY(hipEventRecord(d->ev_w1, d->stream));
    d->wave_timed = true;
    if (sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return ALACGPU_E_OK;
}

int alacgpu_waveform_last_ms(alacgpu_decoder* d, float* ms) {
    if (!d || !ms || !d->wave_timed) {
        set_err(!d || !ms ? "null argument" : "no waveform pass on this handle yet");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipEventSynchronize(d->ev_w1));
    HIP_TRY(hipEventElapsedTime(ms, d->ev_w0, d->ev_w1));
    return ALACGPU_E_OK;
}

int alacgpu_clips_device(alacgpu_decoder* d, const uint8_t* d_pcm, size_t pcm_stride, const uint32_t* d_frames,
                         const int32_t* d_status, size_t n, const uint64_t* d_begin, const uint64_t* d_limit, size_t n_clips,
                         uint32_t clip_frames, int type, void* d_clips, size_t channel_stride, size_t clip_stride,
                         uint32_t* d_valid, int32_t* d_clip_status, int sync) {
    if (!d || (n_clips && (!d_pcm || !d_frames || !d_begin || !d_limit || !d_clips))) {
        set_err("null argument");
        return ALACGPU_E_ARG;
    }
    if (type != ALACGPU_WAVE_FLOAT && type != ALACGPU_WAVE_INT) {
        set_err("unknown waveform type %d", type);
        return ALACGPU_E_ARG;
    }
    if (n > 0x7fffffffu || n_clips > 0x7fffffffu) {
        set_err("batch too large");
        return ALACGPU_E_ARG;
    }
    if (n_clips == 0) return ALACGPU_E_OK;
    const uint64_t ch = d->cfg.num_channels;
    if (clip_frames == 0) {
        set_err("clip_frames is 0");
        return ALACGPU_E_ARG;
    }
    if (n && (pcm_stride < d->frame_bytes || pcm_stride > SIZE_MAX / n)) {
        set_err("pcm_stride %zu < frame bytes %zu, or the slots overflow", pcm_stride, d->frame_bytes);
        return ALACGPU_E_ARG;
    }
    if (reinterpret_cast<uintptr_t>(d_clips) % 4) {
        set_err("d_clips is not aligned to its 4-byte elements");
        return ALACGPU_E_ARG;
    }
    /* every column of a row inside the row, the rows of a clip inside the clip, and the whole tensor countable in bytes */
    if (channel_stride < clip_frames || clip_stride / ch < channel_stride || clip_stride > (SIZE_MAX / 8) / n_clips) {
        set_err("channel_stride %zu / clip_stride %zu too small for clips of %u frames, or the clips overflow", channel_stride, clip_stride,
                clip_frames);
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(d->device));
    alacclip::Params p = alacclip::make_params(d->cfg.frame_length, d->cfg.bit_depth, d->cfg.num_channels, (uint32_t)type, clip_frames);
    p.pcm = d_pcm;
    p.pcm_stride = pcm_stride;
    p.frames = d_frames;
    p.status = d_status;
    p.n = n;
    p.begin = d_begin;
    p.limit = d_limit;
    p.n_clips = n_clips;
    p.clips = (uint8_t*)d_clips;
    p.channel_stride = channel_stride;
    p.clip_stride = clip_stride;
    p.valid = d_valid;
    p.clip_status = d_clip_status;
    HIP_TRY(hipEventRecord(d->ev_c0, d->stream));
    HIP_TRY(alack::clips_launch(d->stream, p));
    HIP_TRY(hipEventRecord(d->ev_c1, d->stream));
    d->clips_timed = true;
    if (sync) HIP_TRY(hipStreamSynchronize(d->stream));
    return ALACGPU_E_OK;
}

int alacgpu_clips_last_ms(alacgpu_decoder* d, float* ms) {
    if (!d || !ms || !d->clips_timed) {
        set_err(!d || !ms ? "null argument" : "no clip gather on this handle yet");
        return ALACGPU_E_ARG;
    }
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipEventSynchronize(d->ev_c1));
    HIP_TRY(hipEventElapsedTime(ms, d->ev_c0, d->ev_c1));
    return ALACGPU_E_OK;
}

void* alacgpu_stream(alacgpu_decoder* d) { return d ? (void*)d->stream : nullptr; }

int alacgpu_synchronize(alacgpu_decoder* d) {
    if (!d) return ALACGPU_E_ARG;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return ALACGPU_E_OK;
}

const char* alacgpu_last_error(void) { return g_err; }

const char* alacgpu_version(void) { return "alacgpu 0.7.0 gfx950"; }

} /* extern "C" */
