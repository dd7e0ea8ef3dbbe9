// kaldi_features.hpp — C++ host-side RAII mirror of the Kaldi feature pass of include/alacgpu.h (alacgpu_fbank_*; the reference
// has no counterpart: it hands out PCM).
//
//   NewKaldiFeatures(config)              -> throws std::invalid_argument where no plan can be built
//   NewKaldiFeatures(config, device, ALACGPU_FBANK_TRANSFORM_FFT)   the opt-in FFT transform (the default is the direct one)
//   FbankConfig(sample_rate, W, h, ...)   an alacgpu_fbank_config with Kaldi's defaults (lengths in samples)
//   MfccConfig(sample_rate, W, h, ...)    the same for MFCC
//   KaldiFeatures::OutFrames(T)           1 + (T - W) / h with snip_edges, (T + h / 2) / h without; 0 for T < W
//   KaldiFeatures::FeaturesDevice(...)    float32 rows on the device -> [rows][F][cols] or [rows][cols][F], asynchronous on
//                                         Stream() unless sync
//   KaldiFeatures::Plan()                 the numbers and the host copies of the tables the kernel uses (an FFT handle has no
//                                         basis: it is empty)
//   KaldiFeatures::FftPlan()              the transform's own numbers and tables (alacgpu_fbank_fft_plan)
// Header-only; link with -lalacgpu. Every pass runs the HIP kernel: there is no CPU path.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

// Kaldi's FbankOptions defaults: 23 bins, povey, 0.97, low_freq 20, energy_floor 1.0; 25 ms / 10 ms frames are W = rate / 40,
// h = rate / 100 where 0 is passed
inline alacgpu_fbank_config FbankConfig(uint32_t sample_rate, uint32_t frame_length = 0, uint32_t frame_shift = 0,
                                        uint32_t num_mel_bins = 23) {
    alacgpu_fbank_config c{};
    c.sample_rate = sample_rate;
    c.frame_length = frame_length ? frame_length : (uint32_t)(sample_rate * 25.0 * 0.001);
    c.frame_shift = frame_shift ? frame_shift : (uint32_t)(sample_rate * 10.0 * 0.001);
    c.round_to_power_of_two = 1;
    c.num_mel_bins = num_mel_bins;
    c.num_ceps = 0;
    c.snip_edges = 1;
    c.remove_dc_offset = 1;
    c.window_type = ALACGPU_FBANK_WINDOW_POVEY;
    c.use_log_fbank = 1;
    c.use_energy = 0;
    c.raw_energy = 1;
    c.htk_compat = 0;
    c.use_power = 1;
    c.log_energy = 1;
    c.layout = ALACGPU_FBANK_LAYOUT_FRAMES;
    c.preemphasis_coefficient = 0.97;
    c.blackman_coeff = 0.42;
    c.low_freq = 20.0;
    c.high_freq = 0.0;
    c.energy_floor = 1.0;
    c.scale = 1.0;
    c.cepstral_lifter = 0.0;
    c.dither = 0.0;
    c.vtln_warp = 1.0;
    return c;
}

// MfccOptions: 13 coefficients, lifter 22
inline alacgpu_fbank_config MfccConfig(uint32_t sample_rate, uint32_t frame_length = 0, uint32_t frame_shift = 0,
                                       uint32_t num_mel_bins = 23, uint32_t num_ceps = 13, double cepstral_lifter = 22.0) {
    alacgpu_fbank_config c = FbankConfig(sample_rate, frame_length, frame_shift, num_mel_bins);
    c.num_ceps = num_ceps;
    c.cepstral_lifter = cepstral_lifter;
    return c;
}

struct KaldiPlan {
    alacgpu_fbank_info info{};
    std::vector<float> basis;   // [2][n_freqs][frame_length]: C, then S, folded
    std::vector<float> fb;      // [num_mel_bins][taps]
    std::vector<int32_t> first; // [num_mel_bins]
    std::vector<float> dct;     // [num_ceps][num_mel_bins]
    std::vector<float> lifter;  // [num_ceps]
};

struct KaldiFftPlan {
    alacgpu_fbank_fft_info info{};
    std::vector<float> window;  // [n_fft]: float(scale * window[n]), zeros from frame_length on
    std::vector<float> twiddle; // 8 roots, each pass's twiddles, the split step's n_fft / 2 + 1 pairs
};

class KaldiFeatures {
public:
    explicit KaldiFeatures(const alacgpu_fbank_config& config, int device = 0, uint32_t transform = ALACGPU_FBANK_TRANSFORM_DIRECT) {
        alacgpu_fbank* h = nullptr;
        detail::check(alacgpu_fbank_create_transform(device, &config, transform, &h));
        h_.reset(h);
    }

    uint64_t OutFrames(uint64_t in_frames) const { return alacgpu_fbank_out_frames(h_.get(), in_frames); }

    // device pointers on the handle's device, strides in elements: rows of in_frames float32 samples -> element (r, f, c) at
    // d_out + r * out_row_stride + f * out_inner_stride + c (layout frames), (r, c, f) at d_out + r * out_row_stride + c *
    // out_inner_stride + f (layout bins); exactly those are written
    void FeaturesDevice(const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out, size_t out_row_stride,
                        size_t out_inner_stride, bool sync = false) {
        detail::check(alacgpu_fbank_device(h_.get(), d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_inner_stride,
                                           sync ? 1 : 0));
    }

    KaldiPlan Plan() const {
        KaldiPlan p;
        detail::must(alacgpu_fbank_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0));
        alacgpu_fbank_fft_info fft{};
        detail::must(alacgpu_fbank_fft_plan(h_.get(), &fft, nullptr, 0, nullptr, 0));
        if (fft.transform == ALACGPU_FBANK_TRANSFORM_DIRECT) p.basis.resize((size_t)2 * p.info.n_freqs * p.info.frame_length);
        p.fb.resize((size_t)p.info.num_mel_bins * p.info.taps);
        p.first.resize(p.info.num_mel_bins);
        p.dct.resize((size_t)p.info.num_ceps * p.info.num_mel_bins);
        p.lifter.resize(p.info.num_ceps);
        detail::must(alacgpu_fbank_plan(h_.get(), &p.info, p.basis.data(), p.basis.size(), p.fb.data(), p.fb.size(), p.first.data(),
                                        p.first.size(), p.dct.data(), p.dct.size(), p.lifter.data(), p.lifter.size()));
        return p;
    }

    KaldiFftPlan FftPlan() const {
        KaldiFftPlan p;
        detail::must(alacgpu_fbank_fft_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0));
        p.window.resize(p.info.window_entries);
        p.twiddle.resize(p.info.twiddle_entries);
        detail::must(alacgpu_fbank_fft_plan(h_.get(), &p.info, p.window.data(), p.window.size(), p.twiddle.data(), p.twiddle.size()));
        return p;
    }

    // milliseconds of the last pass: HIP events around its kernels
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_fbank_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_fbank_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_fbank_synchronize(h_.get())); }
    alacgpu_fbank* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_fbank, alacgpu_fbank_destroy> h_;
};

inline std::unique_ptr<KaldiFeatures> NewKaldiFeatures(const alacgpu_fbank_config& config, int device = 0,
                                                       uint32_t transform = ALACGPU_FBANK_TRANSFORM_DIRECT) {
    return std::make_unique<KaldiFeatures>(config, device, transform);
}

}  // namespace alac
