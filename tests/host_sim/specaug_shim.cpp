/*
 * specaug_shim.cpp — TEST-ONLY C entry points over saprobe-alac_amd/host/spec_augment.hpp, so the Python test-suite can drive it
 * with ctypes (links libalacgpu). specaug_shim_create alone needs no GPU where the configuration is refused.
 */
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/spec_augment.hpp"

extern "C" {

static thread_local char g_msg[1024];
const char* specaug_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* sizeof the header's two structs, the offset of alacgpu_specaug_config's mask_value, and SpecAugConfig's time_ratio_q16 for the
 * ratios 0.2 and 1 */
void specaug_shim_sizes(uint64_t* out) {
    out[0] = sizeof(alacgpu_specaug_config);
    out[1] = sizeof(alacgpu_specaug_info);
    out[2] = offsetof(alacgpu_specaug_config, mask_value);
    out[3] = alac::SpecAugConfig(80, 2, 27, 2, 100, 0.2).time_ratio_q16;
    out[4] = alac::SpecAugConfig(80).time_ratio_q16;
}

/* NewSpecAugment alone: -> 0 (and the handle is closed again), -6 for std::invalid_argument, -5 for anything else */
long specaug_shim_create(const alacgpu_specaug_config* config) {
    try {
        auto sa = alac::NewSpecAugment(*config);
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

/* A SpecAugment for *config, one pass over device pointers (sync), and what it reports: Plan()'s info, LastMs. strides: {row,
 * frame, bin} of the input, then of the output. -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5
 * for anything else */
long specaug_shim_run(const alacgpu_specaug_config* config, const float* d_in, const uint64_t* strides, size_t rows, size_t frames,
                      const int32_t* d_lengths, uint64_t seed, uint64_t row_base, const int64_t* d_ids, float* d_out, int32_t* d_draws,
                      alacgpu_specaug_info* info, float* ms) {
    try {
        auto sa = alac::NewSpecAugment(*config);
        *info = sa->Plan();
        sa->AugmentDevice(d_in, {(size_t)strides[0], (size_t)strides[1], (size_t)strides[2]}, rows, frames, d_lengths, seed, d_out,
                          {(size_t)strides[3], (size_t)strides[4], (size_t)strides[5]}, row_base, d_ids, d_draws, true);
        *ms = sa->LastMs();
        sa->Synchronize();
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
