// wave_augment.hpp — C++ host-side RAII mirror of the waveform augmentation pass of include/alacgpu.h (alacgpu_waveaug_*; the
// reference has no counterpart: it hands out PCM).
//
//   NewWaveAugment(config)              -> throws std::invalid_argument where no plan can be built
//   WaveAugConfig(snr_lo, snr_hi, ...)  an alacgpu_waveaug_config from decibels (rounded to 1 / 256 dB) and a probability
//   NoiseBank                           the device pointers of a bank of noise clips; the default is no noise
//   WaveAugment::AugmentDevice(...)     float32 waveforms on the device with per-row lengths -> gain, noise at an SNR, dither,
//                                       clamp and padding, with the resolved draws and the stats; asynchronous on Stream() unless sync
//   WaveAugment::Plan()                 the parameters, the tile, the scratch block and the two tables
// Header-only; link with -lalacgpu. Every pass runs the HIP kernels: there is no CPU path.
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

// decibels -> 1 / 256 dB; noise_prob in [0, 1] -> 1 / 65536 (anything else: a value that create refuses)
inline alacgpu_waveaug_config WaveAugConfig(double snr_lo = 5.0, double snr_hi = 20.0, double gain_lo = 0.0, double gain_hi = 0.0,
                                            double noise_prob = 1.0, float dither = 0.0f, bool clamp = false, float pad_value = 0.0f) {
    alacgpu_waveaug_config c{};
    c.snr_lo_q8 = (int32_t)std::lround(snr_lo * 256.0);
    c.snr_hi_q8 = (int32_t)std::lround(snr_hi * 256.0);
    c.gain_lo_q8 = (int32_t)std::lround(gain_lo * 256.0);
    c.gain_hi_q8 = (int32_t)std::lround(gain_hi * 256.0);
    c.noise_prob_q16 = noise_prob >= 0.0 && noise_prob <= 1.0 ? (uint32_t)std::lround(noise_prob * 65536.0) : 0xFFFFFFFFu;  // refused
    c.dither = dither;
    c.clamp = clamp ? 1u : 0u;
    c.pad_value = pad_value;
    return c;
}

// rows clips of `samples` floats, `row_stride` elements apart, clip k valid up to d_lengths[k] (null: all of it)
struct NoiseBank {
    const float* d_noise = nullptr;
    size_t row_stride = 0, rows = 0, samples = 0;
    const int32_t* d_lengths = nullptr;
};

struct WaveAugPlan {
    alacgpu_waveaug_info info;
    std::vector<float> snr_amp, gain_amp;
};

class WaveAugment {
public:
    explicit WaveAugment(const alacgpu_waveaug_config& config, int device = 0) {
        alacgpu_waveaug* h = nullptr;
        detail::check(alacgpu_waveaug_create(device, &config, &h));
        h_.reset(h);
    }

    // device pointers on the handle's device: rows x samples elements of d_in -> the same elements of d_out, which may be d_in
    // itself with the same stride (in place) and may not overlap it otherwise, nor the bank. seed: the step's; row r's identity is
    // d_ids[r] (int64 per row) or, where d_ids is null, row_base + r. d_lengths, d_draws (int32 [rows][5]) and d_stats (float
    // [rows][4]) may be null; exactly the output's elements, the draws and the stats are written
    void AugmentDevice(const float* d_in, size_t in_row_stride, size_t rows, size_t samples, const int32_t* d_lengths, uint64_t seed,
                       float* d_out, size_t out_row_stride, const NoiseBank& bank = {}, uint64_t row_base = 0,
                       const int64_t* d_ids = nullptr, int32_t* d_draws = nullptr, float* d_stats = nullptr, bool sync = false) {
        detail::check(alacgpu_waveaug_device(h_.get(), d_in, in_row_stride, rows, samples, d_lengths, bank.d_noise, bank.row_stride,
                                             bank.rows, bank.samples, bank.d_lengths, seed, row_base, d_ids, d_out, out_row_stride,
                                             d_draws, d_stats, sync ? 1 : 0));
    }

    WaveAugPlan Plan() const {
        WaveAugPlan p{};
        detail::must(alacgpu_waveaug_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0));
        p.snr_amp.resize(p.info.snr_entries);
        p.gain_amp.resize(p.info.gain_entries);
        detail::must(alacgpu_waveaug_plan(h_.get(), &p.info, p.snr_amp.data(), p.snr_amp.size(), p.gain_amp.data(), p.gain_amp.size()));
        return p;
    }

    // milliseconds of the last pass: HIP events around its kernels
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_waveaug_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_waveaug_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_waveaug_synchronize(h_.get())); }
    alacgpu_waveaug* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_waveaug, alacgpu_waveaug_destroy> h_;
};

inline std::unique_ptr<WaveAugment> NewWaveAugment(const alacgpu_waveaug_config& config, int device = 0) {
    return std::make_unique<WaveAugment>(config, device);
}

}  // namespace alac
