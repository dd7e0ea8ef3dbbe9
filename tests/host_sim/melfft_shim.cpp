/*
 * melfft_shim.cpp — TEST-ONLY C entry point over the transform member and FftPlan() of
 * saprobe-alac_amd/host/mel_spectrogram.hpp, so the Python test-suite can drive them with ctypes (GPU, links libalacgpu).
 */
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/mel_spectrogram.hpp"

extern "C" {

static thread_local char g_msg[512];
const char* melfft_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* A MelSpectrogram for alac::MelConfig(sample_rate, n_fft, win_length, hop_length, 0, 0, n_mels, center) with its transform
 * member set, FftPlan() (info = the 16 numbers of alacgpu_mel_fft_info; window / twiddle as far as their capacities go, which
 * must suffice), Plan() (a basis of 0 entries with transform = fft, of 2 n_freqs n_fft otherwise) and one pass over device
 * pointers (sync). -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5 for anything else */
long melfft_shim_run(uint32_t sample_rate, uint32_t n_fft, uint32_t win_length, uint32_t hop_length, uint32_t n_mels, int center,
                     uint32_t transform, const float* d_in, size_t in_stride, size_t rows, size_t in_frames, float* d_out,
                     size_t out_row_stride, size_t out_bin_stride, uint32_t* info, float* window, size_t window_cap, float* twiddle,
                     size_t twiddle_cap) {
    try {
        alacgpu_mel_config c = alac::MelConfig(sample_rate, n_fft, win_length, hop_length, 0.0, 0.0, n_mels, center != 0);
        if (c.transform != ALACGPU_MEL_TRANSFORM_DIRECT) return fail(5, "MelConfig's transform does not default to direct");
        c.transform = transform;
        alac::MelSpectrogram mel(c);
        const alac::MelFftPlan pl = mel.FftPlan();
        static_assert(sizeof(pl.info) == 16 * sizeof(uint32_t), "alacgpu_mel_fft_info");
        memcpy(info, &pl.info, sizeof(pl.info));
        if (pl.window.size() > window_cap || pl.twiddle.size() > twiddle_cap) return fail(5, "capacity below the plan");
        memcpy(window, pl.window.data(), pl.window.size() * sizeof(float));
        memcpy(twiddle, pl.twiddle.data(), pl.twiddle.size() * sizeof(float));
        const alac::MelPlan mp = mel.Plan(); /* an FFT handle has no basis; filterbank and tile are reported as ever */
        const size_t basis = transform == ALACGPU_MEL_TRANSFORM_FFT ? 0 : (size_t)2 * mp.info.n_freqs * mp.info.n_fft;
        if (mp.basis.size() != basis) return fail(5, "Plan(): the basis has not the entries its transform has");
        if (mp.fb.size() != (size_t)n_mels * mp.info.taps || mp.first.size() != n_mels || mp.info.tile_frames != pl.info.tile_frames ||
            mp.info.lds_bytes != pl.info.lds_bytes)
            return fail(5, "Plan() and FftPlan() disagree");
        mel.MelDevice(d_in, in_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride, true);
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
