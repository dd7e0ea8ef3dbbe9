/*
 * waveaug_shim.cpp — TEST-ONLY C entry points over saprobe-alac_amd/host/wave_augment.hpp, so the Python test-suite can drive it
 * with ctypes (links libalacgpu). waveaug_shim_create alone needs no GPU where the configuration is refused.
 */
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/wave_augment.hpp"

extern "C" {

static thread_local char g_msg[1024];
const char* waveaug_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* sizeof the header's two structs, the offsets of alacgpu_waveaug_config's dither and alacgpu_waveaug_info's scratch_bytes, and
 * WaveAugConfig's fields for (5, 20) dB SNR, (-6, 3) dB gain and a probability of 0.8: snr_hi_q8, gain_lo_q8 (as it is stored in
 * 64 bits), noise_prob_q16 */
void waveaug_shim_sizes(int64_t* out) {
    out[0] = sizeof(alacgpu_waveaug_config);
    out[1] = sizeof(alacgpu_waveaug_info);
    out[2] = offsetof(alacgpu_waveaug_config, dither);
    out[3] = offsetof(alacgpu_waveaug_info, scratch_bytes);
    const alacgpu_waveaug_config c = alac::WaveAugConfig(5, 20, -6, 3, 0.8);
    out[4] = c.snr_hi_q8;
    out[5] = c.gain_lo_q8;
    out[6] = c.noise_prob_q16;
}

/* NewWaveAugment alone: -> 0 (and the handle is closed again), -6 for std::invalid_argument, -5 for anything else */
long waveaug_shim_create(const alacgpu_waveaug_config* config) {
    try {
        auto wa = alac::NewWaveAugment(*config);
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

/* A WaveAugment for *config, one pass over device pointers (sync), and what it reports: Plan()'s info and the first entry of
 * each table in tables[2], LastMs. -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5 for anything
 * else */
long waveaug_shim_run(const alacgpu_waveaug_config* config, const float* d_in, size_t in_rs, size_t rows, size_t samples,
                      const int32_t* d_lengths, const float* d_noise, size_t noise_rs, size_t noise_rows, size_t noise_samples,
                      const int32_t* d_noise_lengths, uint64_t seed, uint64_t row_base, const int64_t* d_ids, float* d_out, size_t out_rs,
                      int32_t* d_draws, float* d_stats, alacgpu_waveaug_info* info, float* tables_and_ms) {
    try {
        auto wa = alac::NewWaveAugment(*config);
        alac::NoiseBank bank;
        bank.d_noise = d_noise;
        bank.row_stride = noise_rs;
        bank.rows = noise_rows;
        bank.samples = noise_samples;
        bank.d_lengths = d_noise_lengths;
        wa->AugmentDevice(d_in, in_rs, rows, samples, d_lengths, seed, d_out, out_rs, bank, row_base, d_ids, d_draws, d_stats, true);
        const alac::WaveAugPlan plan = wa->Plan();
        *info = plan.info;
        tables_and_ms[0] = plan.snr_amp.at(0);
        tables_and_ms[1] = plan.gain_amp.at(0);
        tables_and_ms[2] = wa->LastMs();
        wa->Synchronize();
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
