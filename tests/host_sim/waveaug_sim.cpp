/*
 * waveaug_sim.cpp — TEST-ONLY host build of the waveform augmentation pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_waveaug.h (the text the gfx950 kernels of k_waveaug.hip are built from) with g++, contraction
 * off, and runs it the way k_waveaug.hip launches it: for every workgroup each phase for work items 0..255 with the barriers
 * between them, the partials kernel, the finish kernel and the apply kernel one after the other. The LDS block is a heap block of
 * exactly the kernels' size, filled with a pattern before every workgroup; the scratch block has exactly scratch_floats_of's
 * floats. The CPU suite (-m "not gpu") checks it against a numpy restatement, and the GPU suite holds the kernels to it. It lives
 * under tests/ and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../saprobe-alac_amd/csrc/alac_waveaug.h"

using namespace alacwa;

extern "C" {

/* cfg = {snr_lo_q8, snr_hi_q8, gain_lo_q8, gain_hi_q8, noise_prob_q16, clamp} */
static Config config_of(const int32_t* cfg, float dither, float pad_value) {
    return Config{cfg[0], cfg[1], cfg[2], cfg[3], (uint32_t)cfg[4], dither, (uint32_t)cfg[5], pad_value};
}

/* one Philox4x32-10 block through this header's include: counter[4], key[2] -> out[4] */
void waveaug_sim_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
    philox4x32_10(c, key[0], key[1]);
    memcpy(out, c, sizeof(c));
}

/* alacgpu_waveaug_create's check + alacgpu_waveaug_plan's numbers and tables: info = {tile, draws, snr_entries, gain_entries,
 * lds_bytes}; the tables where the pointers are not NULL (the caller sizes them by a first call). -> 0, or -2 where create is
 * ALACGPU_E_ARG */
int waveaug_sim_plan(const int32_t* cfg, float dither, uint32_t* info, float* snr_out, float* gain_out) {
    const Config c = config_of(cfg, dither, 0.0f);
    if (!info || !config_ok(c)) return -2;
    const std::vector<float> s = snr_table(c), g = gain_table(c);
    info[0] = kTile;
    info[1] = kDraws;
    info[2] = (uint32_t)s.size();
    info[3] = (uint32_t)g.size();
    info[4] = kLdsFloats * 4u;
    if (snr_out) memcpy(snr_out, s.data(), s.size() * sizeof(float));
    if (gain_out) memcpy(gain_out, g.data(), g.size() * sizeof(float));
    return 0;
}

/* The arguments of alacgpu_waveaug_create and alacgpu_waveaug_device with host pointers. -> 0, or -2 for what the entries reject. */
int waveaug_sim_run(const int32_t* cfg, float dither, float pad_value, const float* in, uint64_t in_rs, uint64_t rows, uint64_t T,
                    const int32_t* lengths, const float* noise, uint64_t noise_rs, uint64_t noise_rows, uint64_t noise_T,
                    const int32_t* noise_lengths, uint64_t seed, uint64_t row_base, const int64_t* ids, float* out, uint64_t out_rs,
                    int32_t* draws, float* stats) {
    const Config c = config_of(cfg, dither, pad_value);
    if (!config_ok(c)) return -2;
    if (rows == 0 || T == 0) return 0;
    const std::vector<float> snr = snr_table(c), gain = gain_table(c);
    Params p;
    uint64_t floats = 0;
    if (!make_params(c, snr.data(), gain.data(), in, in_rs, rows, T, lengths, noise, noise_rs, noise_rows, noise_T, noise_lengths, seed,
                     row_base, ids, out, out_rs, draws, stats, &p) ||
        !scratch_floats_of(rows, T, p.reduce != 0u, stats == nullptr, &floats))
        return -2;
    std::vector<float> scratch(floats);
    if (floats) memset(scratch.data(), 0xFF, floats * sizeof(float)); /* NaN wherever a kernel reads what none wrote */
    set_scratch(&p, scratch.data());
    std::vector<float> lds(kLdsFloats);
    const auto each = [](auto&& phase) {
        for (uint32_t tid = 0; tid < kThreads; tid++) phase(tid);
    };
    const auto fresh = [&] { memset(lds.data(), 0xA5, lds.size() * sizeof(float)); }; /* LDS holds whatever the last workgroup left */
    if (p.reduce) {
        for (uint64_t row = 0; row < rows; row++)
            for (uint64_t chunk = 0; chunk < p.chunks; chunk++) { /* alac_waveaug_partials */
                const Chunk ck = make_chunk(p, row, chunk);
                if (ck.nv == 0u) continue;
                fresh();
                const Lds l = carve(lds.data(), kTile);
                each([&](uint32_t tid) {
                    lines_in(ck.x, 0u, 1u, ck.nv, l.image, 0u, 1u, tid);
                    row_words(p, ck.id, l.words, tid);
                });
                const Draws d = resolve(p, l.words);
                each([&](uint32_t tid) { l.lanes[tid] = lane_sum(l.image, ck.nv, tid); });
                each([&](uint32_t tid) {
                    if (d.applied) stage_noise(p, ck, d, l.image, tid);
                });
                each([&](uint32_t tid) { l.lanes[kThreads + tid] = d.applied ? lane_sum(l.image, ck.nv, tid) : 0.0f; });
                for (uint32_t s = kThreads / 2u; s > 0u; s >>= 1) each([&](uint32_t tid) { fold(l.lanes, s, tid); });
                each([&](uint32_t tid) { put_partials(p, ck, l.lanes, tid); });
            }
        for (uint64_t row = 0; row < rows; row++) { /* alac_waveaug_finish */
            fresh();
            const Lds l = carve(lds.data(), 0u);
            const uint64_t nc = chunks_of(p, row);
            each([&](uint32_t tid) {
                finish_start(l.sums, tid);
                row_words(p, id_of(p, row), l.words, tid);
            });
            for (uint64_t c0 = 0; c0 < nc; c0 += kThreads) {
                const uint32_t cnt = nc - c0 < kThreads ? (uint32_t)(nc - c0) : kThreads;
                each([&](uint32_t tid) { finish_load(p, row, c0, cnt, l.lanes, tid); });
                each([&](uint32_t tid) { finish_add(l.lanes, cnt, l.sums, tid); });
            }
            each([&](uint32_t tid) { finish_row(p, row, l, tid); });
        }
    }
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t chunk = 0; chunk < p.chunks; chunk++) { /* alac_waveaug_apply / alac_waveaug_apply_dither */
            const Chunk ck = make_chunk(p, row, chunk);
            fresh();
            const Lds l = carve(lds.data(), kTile);
            each([&](uint32_t tid) { row_words(p, ck.id, l.words, tid); });
            const Draws d = resolve(p, l.words);
            const float a = gain_of(p, d);
            const float nb = p.reduce ? p.stats[row * kStats + 3u] : 0.0f;
            each([&](uint32_t tid) {
                if (nb != 0.0f && ck.nv) stage_noise(p, ck, d, l.image, tid);
                if (!p.reduce && p.draws_out && ck.t0 == 0u && tid == 0u) put_draws(p, row, d);
            });
            each([&](uint32_t tid) {
                if (p.dither != 0.0f) apply_chunk<true>(p, ck, a, nb, l.image, tid);
                else apply_chunk<false>(p, ck, a, nb, l.image, tid);
            });
        }
    return 0;
}

}  // extern "C"
