/*
 * stack_shim.cpp — TEST-ONLY C entry points over saprobe-alac_amd/host/frame_stack.hpp, so the Python test-suite can drive it
 * with ctypes (links libalacgpu). stack_shim_create alone needs no GPU where the configuration is refused.
 */
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/host/frame_stack.hpp"

extern "C" {

static thread_local char g_msg[1024];
const char* stack_shim_last_error() { return g_msg; }

static int fail(int kind, const char* what) {
    strncpy(g_msg, what, sizeof(g_msg) - 1);
    return -kind;
}

/* sizeof the header's two structs, and the offset of alacgpu_stack_config's pad_value */
void stack_shim_sizes(uint64_t* out) {
    out[0] = sizeof(alacgpu_stack_config);
    out[1] = sizeof(alacgpu_stack_info);
    out[2] = offsetof(alacgpu_stack_config, pad_value);
}

/* NewFrameStack alone: -> 0 (and the handle is closed again), -6 for std::invalid_argument, -5 for anything else */
long stack_shim_create(const alacgpu_stack_config* config) {
    try {
        auto fs = alac::NewFrameStack(*config);
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

/* A FrameStack for *config, one pass over device pointers (sync), and what it reports: OutFrames(frames), the thirteen numbers of
 * Plan()'s info, its tables' sizes, LastMs. strides: {row, frame, bin} of the input, then of the output.
 * -> 0, -6 for std::invalid_argument (no plan, or arguments the pass refuses), -5 for anything else */
long stack_shim_run(const alacgpu_stack_config* config, const float* d_in, const uint64_t* strides, size_t rows, size_t frames,
                    const int32_t* d_lengths, float* d_out, int32_t* d_out_lengths, uint64_t* out_frames, uint32_t* info,
                    uint64_t* table_sizes, float* ms) {
    try {
        auto fs = alac::NewFrameStack(*config);
        *out_frames = fs->OutFrames(frames);
        const alac::StackPlan pl = fs->Plan();
        memcpy(info, &pl.info, sizeof(pl.info));
        table_sizes[0] = pl.w1.size();
        table_sizes[1] = pl.w2.size();
        fs->StackDevice(d_in, {(size_t)strides[0], (size_t)strides[1], (size_t)strides[2]}, rows, frames, d_lengths, d_out,
                        {(size_t)strides[3], (size_t)strides[4], (size_t)strides[5]}, d_out_lengths, true);
        *ms = fs->LastMs();
        fs->Synchronize();
    } catch (const std::invalid_argument& e) { return fail(6, e.what());
    } catch (const std::exception& e) { return fail(5, e.what()); }
    return 0;
}

}  // extern "C"
