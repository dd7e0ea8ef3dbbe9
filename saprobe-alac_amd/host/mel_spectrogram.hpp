// mel_spectrogram.hpp — C++ host-side RAII mirror of the spectrogram pass of include/alacgpu.h (alacgpu_mel_*; the reference
// has no counterpart: it hands out PCM).
//
//   NewMelSpectrogram(config)             -> throws std::invalid_argument where no plan can be built
//   MelConfig(sample_rate, n_fft, ...)    an alacgpu_mel_config with torchaudio's defaults resolved
//   MelSpectrogram::OutFrames(T)          1 + (T - n_fft % 2) / hop centred, 1 + (T - n_fft) / hop otherwise; 0 where no frame exists
//   MelSpectrogram::MelDevice(...)        float32 rows on the device -> [rows][bins][frames], asynchronous on Stream() unless sync
//   MelSpectrogram::Plan()                the numbers and the host copies of the tables the kernel uses
//   MelConfig(...).transform              ALACGPU_MEL_TRANSFORM_DIRECT (the default) or _FFT: n_fft even, n_fft / 2 = 2^a 3^b 5^c
//   MelSpectrogram::FftPlan()             the FFT's numbers, window and twiddle table (transform 0 and no tables on a direct handle)
// Header-only; link with -lalacgpu. Every pass runs the HIP kernel: there is no CPU path.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/alacgpu.h"
#include "pass_handle.hpp"

namespace alac {

// win_length 0: n_fft; hop_length 0: win_length / 2; f_max <= 0: sample_rate / 2; n_mels 0: the power spectrogram itself
inline alacgpu_mel_config MelConfig(uint32_t sample_rate, uint32_t n_fft = 400, uint32_t win_length = 0, uint32_t hop_length = 0,
                                    double f_min = 0.0, double f_max = 0.0, uint32_t n_mels = 128, bool center = true,
                                    bool slaney_norm = false, int mel_scale = ALACGPU_MEL_SCALE_HTK, int log = ALACGPU_MEL_LOG_NONE,
                                    double floor = 1e-10) {
    alacgpu_mel_config c{};
    c.sample_rate = sample_rate;
    c.n_fft = n_fft;
    c.win_length = win_length ? win_length : n_fft;
    c.hop_length = hop_length ? hop_length : c.win_length / 2;
    c.f_min = f_min;
    c.f_max = f_max > 0.0 ? f_max : sample_rate / 2.0;
    c.n_mels = n_mels;
    c.center = center ? 1u : 0u;
    c.norm = n_mels && slaney_norm ? 1u : 0u;
    c.mel_scale = n_mels ? (uint32_t)mel_scale : (uint32_t)ALACGPU_MEL_SCALE_NONE;
    c.log = (uint32_t)log;
    c.transform = ALACGPU_MEL_TRANSFORM_DIRECT;
    c.floor = floor;
    return c;
}

struct MelPlan {
    alacgpu_mel_info info{};
    std::vector<float> basis;   // [2][n_freqs][n_fft]: C, then S; empty on a handle with transform = fft
    std::vector<float> fb;      // [n_mels][taps]
    std::vector<int32_t> first; // [n_mels]: the bin of each filter window's first weight
};

struct MelFftPlan {
    alacgpu_mel_fft_info info{};
    std::vector<float> window;  // [n_fft]
    std::vector<float> twiddle; // roots, the passes' twiddles, the split step's (include/alacgpu.h)
};

class MelSpectrogram {
public:
    explicit MelSpectrogram(const alacgpu_mel_config& config, int device = 0) {
        alacgpu_mel* h = nullptr;
        detail::check(alacgpu_mel_create(device, &config, &h));
        h_.reset(h);
    }

    uint64_t OutFrames(uint64_t in_frames) const { return alacgpu_mel_out_frames(h_.get(), in_frames); }

    // device pointers on the handle's device, strides in elements: rows of in_frames float32 samples -> element (r, b, f) at
    // d_out + r * out_row_stride + b * out_bin_stride + f for b < bins, f < OutFrames(in_frames); exactly those are written
    void MelDevice(const float* d_in, size_t in_row_stride, size_t rows, size_t in_frames, float* d_out, size_t out_row_stride,
                   size_t out_bin_stride, bool sync = false) {
        detail::check(alacgpu_mel_device(h_.get(), d_in, in_row_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride,
                                         sync ? 1 : 0));
    }

    MelPlan Plan() const {
        MelPlan p;
        detail::must(alacgpu_mel_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0, nullptr, 0));
        alacgpu_mel_fft_info fft{};
        detail::must(alacgpu_mel_fft_plan(h_.get(), &fft, nullptr, 0, nullptr, 0));
        // a handle with transform = fft builds no basis: 0 entries
        p.basis.resize(fft.transform == ALACGPU_MEL_TRANSFORM_DIRECT ? (size_t)2 * p.info.n_freqs * p.info.n_fft : 0);
        p.fb.resize((size_t)p.info.n_mels * p.info.taps);
        p.first.resize(p.info.n_mels);
        detail::must(alacgpu_mel_plan(h_.get(), &p.info, p.basis.data(), p.basis.size(), p.fb.data(), p.fb.size(), p.first.data(),
                                      p.first.size()));
        return p;
    }

    MelFftPlan FftPlan() const {
        MelFftPlan p;
        detail::must(alacgpu_mel_fft_plan(h_.get(), &p.info, nullptr, 0, nullptr, 0));
        p.window.resize(p.info.window_entries);
        p.twiddle.resize(p.info.twiddle_entries);
        detail::must(alacgpu_mel_fft_plan(h_.get(), &p.info, p.window.data(), p.window.size(), p.twiddle.data(), p.twiddle.size()));
        return p;
    }

    // milliseconds of the last pass: HIP events around its kernels
    float LastMs() {
        float ms = 0;
        detail::must(alacgpu_mel_last_ms(h_.get(), &ms));
        return ms;
    }

    void* Stream() const { return alacgpu_mel_stream(h_.get()); }
    void Synchronize() { detail::must(alacgpu_mel_synchronize(h_.get())); }
    alacgpu_mel* handle() const { return h_.get(); }

private:
    detail::Handle<alacgpu_mel, alacgpu_mel_destroy> h_;
};

inline std::unique_ptr<MelSpectrogram> NewMelSpectrogram(const alacgpu_mel_config& config, int device = 0) {
    return std::make_unique<MelSpectrogram>(config, device);
}

}  // namespace alac
