/*
 * fbankfft_shim.cpp — TEST-ONLY C entry point over saprobe-alac_amd/host/kaldi_features.hpp with a transform, so the Python
 * test-suite can drive it with ctypes (GPU, links libalacgpu).
 */
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/kaldi_features.hpp"

extern "C" {

static thread_local char g_msg[1024];
const char* fbankfft_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* A KaldiFeatures for *config with `transform`, one pass over device pointers (sync), and what it reports: OutFrames, the ten
 * numbers of Plan()'s info, the size of its basis, the sixteen numbers of FftPlan()'s info and its tables' sizes, LastMs.
 * -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5 for anything else */
long fbankfft_shim_run(const alacgpu_fbank_config* config, uint32_t transform, const float* d_in, size_t in_stride, size_t rows,
                       size_t in_frames, float* d_out, size_t out_row_stride, size_t out_inner_stride, uint64_t* out_frames,
                       uint32_t* info, uint64_t* basis_size, uint32_t* fft_info, uint64_t* table_sizes, float* ms) {
    try {
        auto kf = alac::NewKaldiFeatures(*config, 0, transform);
        *out_frames = kf->OutFrames(in_frames);
        const alac::KaldiPlan pl = kf->Plan();
        memcpy(info, &pl.info, 10 * sizeof(uint32_t));
        *basis_size = pl.basis.size();
        const alac::KaldiFftPlan fp = kf->FftPlan();
        memcpy(fft_info, &fp.info, 16 * sizeof(uint32_t));
        table_sizes[0] = fp.window.size();
        table_sizes[1] = fp.twiddle.size();
        kf->FeaturesDevice(d_in, in_stride, rows, in_frames, d_out, out_row_stride, out_inner_stride, true);
        *ms = kf->LastMs();
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
