/*
 * mel_shim.cpp — TEST-ONLY C entry point over saprobe-alac_amd/host/mel_spectrogram.hpp, so the Python test-suite can drive it
 * with ctypes (GPU, links libalacgpu).
 */
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/mel_spectrogram.hpp"

extern "C" {

static thread_local char g_msg[512];
const char* mel_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* A MelSpectrogram for alac::MelConfig(the arguments), one pass over device pointers (sync), and what it reports: OutFrames,
 * Plan (info = the nine numbers of alacgpu_mel_info; basis / fb / first as far as their capacities go, which must suffice) and
 * LastMs. -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5 for anything else */
long mel_shim_run(uint32_t sample_rate, uint32_t n_fft, uint32_t win_length, uint32_t hop_length, double f_min, double f_max,
                  uint32_t n_mels, int center, int slaney_norm, int mel_scale, int log, double floor, const float* d_in,
                  size_t in_stride, size_t rows, size_t in_frames, float* d_out, size_t out_row_stride, size_t out_bin_stride,
                  uint64_t* out_frames, uint32_t* info, float* basis, size_t basis_cap, float* fb, size_t fb_cap, int32_t* first,
                  size_t first_cap, float* ms) {
    try {
        alac::MelSpectrogram mel(alac::MelConfig(sample_rate, n_fft, win_length, hop_length, f_min, f_max, n_mels, center != 0,
                                                 slaney_norm != 0, mel_scale, log, floor));
        *out_frames = mel.OutFrames(in_frames);
        const alac::MelPlan pl = mel.Plan();
        memcpy(info, &pl.info, 9 * sizeof(uint32_t));
        if (pl.basis.size() > basis_cap || pl.fb.size() > fb_cap || pl.first.size() > first_cap) return fail(5, "capacity below the plan");
        memcpy(basis, pl.basis.data(), pl.basis.size() * sizeof(float));
        memcpy(fb, pl.fb.data(), pl.fb.size() * sizeof(float));
        memcpy(first, pl.first.data(), pl.first.size() * sizeof(int32_t));
        mel.MelDevice(d_in, in_stride, rows, in_frames, d_out, out_row_stride, out_bin_stride, true);
        *ms = mel.LastMs();
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
