/*
 * enc_sim.cpp — TEST-ONLY host build of the encoder's per-lane logic.
 *
 * Compiles saprobe-alac_amd/csrc/alac_enc.h (the text the gfx950 encode kernels are built from) with g++ and runs its
 * stages the way k_enc.hip launches them: a chain encode per (packet, chain), a layout per packet, an exclusive scan of
 * the sizes, and the pack stage one output dword at a time (byte stores at a packet's unaligned ends). The CPU suite
 * (-m "not gpu") checks this against the oracle; the GPU suite checks the kernels' bytes against it; tools/encode_bench.py
 * times it on threads as the CPU baseline. It lives under tests/ and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../saprobe-alac_amd/csrc/alac_enc.h"

using namespace alacenc;

namespace {

template <class F>
void parallel_for(uint64_t n, int threads, F f) {
    if (threads < 1) threads = 1;
    if ((uint64_t)threads > n) threads = n ? (int)n : 1;
    std::vector<std::thread> pool;
    const uint64_t per = (n + (uint64_t)threads - 1) / (uint64_t)threads;
    for (int t = 0; t < threads; t++) {
        const uint64_t lo = (uint64_t)t * per, hi = lo + per < n ? lo + per : n;
        if (threads == 1) {
            for (uint64_t i = lo; i < hi; i++) f(i);
        } else {
            pool.emplace_back([=] {
                for (uint64_t i = lo; i < hi; i++) f(i);
            });
        }
    }
    for (auto& th : pool) th.join();
}

}  // namespace

extern "C" {

uint64_t enc_sim_max_bytes(const alacgpu_config* cfg, uint64_t total_frames) { return max_bytes(*cfg, total_frames); }

void enc_sim_cookie(const alacgpu_config* cfg, uint32_t max_frame_bytes, uint32_t avg_bit_rate, uint8_t* out) {
    cookie(*cfg, max_frame_bytes, avg_bit_rate, out);
}

/* -> packets, or -1 when blob_cap < max_bytes. offsets: n + 1 entries. escaped (may be NULL): per packet, bit e = element e
 * went out raw. elem_starts (may be NULL): per packet, 5 entries, the bit where element e's header starts. */
long enc_sim_encode(const alacgpu_config* cfg, const uint8_t* pcm, uint64_t total_frames, uint8_t* blob, uint64_t blob_cap,
                    uint64_t* offsets, uint32_t* escaped, uint64_t* elem_starts, int threads) {
    if (blob_cap < max_bytes(*cfg, total_frames)) return -1;
    const Params p = make_params(*cfg, total_frames);
    const uint64_t n = p.n_packets;
    std::vector<ChainResult> res(n * p.nch);
    std::vector<uint32_t> streams(n * p.nch * p.chain_words + 1);
    parallel_for(n * p.nch, threads, [&](uint64_t t) {
        const uint64_t pk = t / p.nch;
        encode_chain(p, pcm, pk, (uint32_t)(t % p.nch), streams.data() + t * p.chain_words, &res[t]);
    });
    std::vector<Layout> lay(n);
    parallel_for(n, threads, [&](uint64_t pk) {
        build_layout(p, pk, res.data() + pk * p.nch, pk * p.nch * p.chain_words, &lay[pk]);
    });
    offsets[0] = 0;
    for (uint64_t pk = 0; pk < n; pk++) offsets[pk + 1] = offsets[pk] + lay[pk].bytes;
    parallel_for(n, threads, [&](uint64_t pk) {
        const uint64_t off = offsets[pk], end = off + lay[pk].bytes;
        uint32_t cursor = 0;
        for (uint64_t D = off / 4; D * 4 < end; D++) {
            const uint32_t v = window(p, lay[pk], streams.data(), pcm, 8 * ((int64_t)(D * 4) - (int64_t)off), cursor);
            for (int k = 0; k < 4; k++) {
                const uint64_t a = D * 4 + (uint64_t)k;
                if (a >= off && a < end) blob[a] = (uint8_t)(v >> (24 - 8 * k));
            }
        }
        if (escaped) escaped[pk] = lay[pk].escaped;
        if (elem_starts)
            for (uint32_t i = 0; i < lay[pk].nseg; i++) {
                const Seg& sg = lay[pk].seg[i];
                if ((sg.kind & 0xffu) == kSegLit && sg.arg < (uint64_t)kMaxElems * kHdrWords)
                    elem_starts[pk * kMaxElems + sg.arg / kHdrWords] = sg.start;
            }
    });
    return (long)n;
}

}  // extern "C"
