/*
 * featnorm_shim.cpp — TEST-ONLY C entry points over saprobe-alac_amd/host/feature_norm.hpp, so the Python test-suite can drive
 * it with ctypes (links libalacgpu). featnorm_shim_create alone needs no GPU where the configuration is refused.
 */
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/feature_norm.hpp"

extern "C" {

static thread_local char g_msg[1024];
const char* featnorm_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* sizeof the header's two structs, and the offset of alacgpu_norm_info's first 64-bit field */
void featnorm_shim_sizes(uint64_t* out) {
    out[0] = sizeof(alacgpu_norm_config);
    out[1] = sizeof(alacgpu_norm_info);
    out[2] = offsetof(alacgpu_norm_info, scratch_bytes);
}

/* NewFeatureNorm alone: -> 0 (and the handle is closed again), -6 for std::invalid_argument, -5 for anything else */
long featnorm_shim_create(const alacgpu_norm_config* config, const float* shift, uint64_t n_shift, const float* scale,
                          uint64_t n_scale) {
    try {
        auto fn = alac::NewFeatureNorm(*config, std::vector<float>(shift, shift + n_shift), std::vector<float>(scale, scale + n_scale));
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

/* A FeatureNorm for *config, one pass over device pointers (sync), and what it reports: OutFrames(frames), the six numbers of
 * Plan()'s info, its tables' sizes, LastMs. strides: {row, frame, bin} of the input, then of the output.
 * -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5 for anything else */
long featnorm_shim_run(const alacgpu_norm_config* config, const float* shift, const float* scale, const float* d_in,
                       const uint64_t* strides, size_t rows, size_t frames, const int32_t* d_lengths, float* d_out, float* d_stats,
                       uint64_t* out_frames, uint32_t* info, uint64_t* table_sizes, float* ms) {
    try {
        const std::vector<float> sh(shift, shift + (shift ? config->bins : 0)), sc(scale, scale + (scale ? config->bins : 0));
        auto fn = alac::NewFeatureNorm(*config, sh, sc);
        *out_frames = fn->OutFrames(frames);
        const alac::NormPlan pl = fn->Plan();
        memcpy(info, &pl.info, 6 * sizeof(uint32_t));
        table_sizes[0] = pl.shift.size();
        table_sizes[1] = pl.scale.size();
        fn->NormDevice(d_in, {(size_t)strides[0], (size_t)strides[1], (size_t)strides[2]}, rows, frames, d_lengths, d_out,
                       {(size_t)strides[3], (size_t)strides[4], (size_t)strides[5]}, d_stats, true);
        *ms = fn->LastMs();
        fn->Synchronize();
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
