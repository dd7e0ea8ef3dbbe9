/*
 * featnorm_sim.cpp — TEST-ONLY host build of the feature normalisation pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_featnorm.h (the text the gfx950 kernels of k_featnorm.hip are built from) with g++,
 * contraction off, and runs it the way k_featnorm.hip launches it: the launches of alacfn::for_each_launch in order, for every
 * workgroup of a launch each phase for work items 0..255 with the barriers between them. The LDS image is a heap block of
 * exactly the plan's size, filled with a pattern before every workgroup. The CPU suite (-m "not gpu") checks it against a numpy
 * restatement, and the GPU suite holds the kernels to it. It lives under tests/ and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../saprobe-alac_amd/csrc/alac_featnorm.h"

using namespace alacfn;

extern "C" {

/* alacgpu_norm_create's check + alacgpu_norm_plan's numbers: info = {tile_frames, lds_bytes}. -> 0, or -2 where create is
 * ALACGPU_E_ARG */
int featnorm_sim_plan(uint32_t bins, uint32_t stat, float var_floor, float range, uint32_t* info) {
    const Config c{bins, stat, var_floor, range, 0.0f};
    if (!info || !config_ok(c)) return -2;
    info[0] = tile_frames_of(bins);
    info[1] = lds_floats_of(bins, info[0]) * (uint32_t)sizeof(float);
    return 0;
}

/* The arguments of alacgpu_norm_create and alacgpu_norm_device with host pointers. -> 0, or -2 for what the entries reject. */
int featnorm_sim_run(uint32_t bins, uint32_t stat, float var_floor, float range, float pad_value, const float* shift,
                     const float* scale, const float* in, uint64_t in_rs, uint64_t in_fs, uint64_t in_bs, uint64_t rows,
                     uint64_t frames, const int32_t* lengths, float* out, uint64_t out_rs, uint64_t out_fs, uint64_t out_bs,
                     float* stats) {
    const Config c{bins, stat, var_floor, range, pad_value};
    if (!config_ok(c)) return -2;
    if (rows == 0 || frames == 0) return 0;
    uint64_t floats = 0;
    if (!scratch_floats_of(c, rows, frames, stats == nullptr, &floats)) return -2;
    std::vector<float> scratch(floats + 1u, -7.0f);
    Params p;
    if (!make_params(c, in, in_rs, in_fs, in_bs, rows, frames, lengths, out, out_rs, out_fs, out_bs, stats, shift, scale, &p))
        return -2;
    set_scratch(&p, scratch.data());
    if (stats && stat == kNone) memset(stats, 0, (size_t)(rows * 2u * bins) * sizeof(float));
    const uint32_t lds_floats = lds_floats_of(p.bins, p.tile_frames);
    std::vector<float> lds(lds_floats);
    int32_t* red = (int32_t*)(lds.data() + image_floats_of(p.bins, p.tile_frames));
    const auto each = [](auto&& phase) {
        for (uint32_t tid = 0; tid < kThreads; tid++) phase(tid);
    };
    for_each_launch(stat, [&](uint32_t kernel, uint32_t phase) {
        Params q = p;
        q.phase = phase;
        if (kernel == 1u && phase != kLargest) {
            for (uint64_t row = 0; row < rows; row++)
                for (uint32_t b = 0; b < bins; b++) finish_bin(q, row, b);
            return;
        }
        if (kernel == 1u) {
            for (uint64_t row = 0; row < rows; row++) {
                memset(red, 0xA5, kRed * sizeof(int32_t));
                each([&](uint32_t tid) { row_max(q, row, red, tid); });
                each([&](uint32_t tid) { reduce_keys(red, 0u, tid); });
                each([&](uint32_t tid) { reduce_keys(red, 1u, tid); });
                each([&](uint32_t tid) { put_row_max(q, row, red, tid); });
            }
            return;
        }
        for (uint64_t row = 0; row < rows; row++)
            for (uint64_t chunk = 0; chunk < q.chunks; chunk++) {
                const Tile t = make_tile(q, row, chunk);
                memset(lds.data(), 0xA5, lds_floats * sizeof(float)); /* LDS holds whatever the last workgroup left */
                if (kernel == 0u) {
                    if (t.nv == 0) continue;
                    each([&](uint32_t tid) { stage_tile(q, t, lds.data(), tid); });
                    if (phase != kLargest) {
                        each([&](uint32_t tid) { sum_tile(q, t, lds.data(), tid); });
                        continue;
                    }
                    each([&](uint32_t tid) { max_tile(q, t, lds.data(), red, tid); });
                    each([&](uint32_t tid) { reduce_keys(red, 0u, tid); });
                    each([&](uint32_t tid) { reduce_keys(red, 1u, tid); });
                    each([&](uint32_t tid) { put_tile_max(q, t, red, tid); });
                } else {
                    if (t.nv) each([&](uint32_t tid) { stage_tile(q, t, lds.data(), tid); });
                    each([&](uint32_t tid) { apply_tile(q, t, lds.data(), tid); });
                    each([&](uint32_t tid) { store_tile(q, t, lds.data(), tid); });
                }
            }
    });
    return 0;
}

}  // extern "C"
