/*
 * stack_sim.cpp — TEST-ONLY host build of the frame stacking pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_stack.h (the text the gfx950 kernel of k_stack.hip is built from) with g++, contraction
 * off, and runs it the way k_stack.hip launches it: for every workgroup (row, tile) each phase for work items 0..255 with the
 * barriers between them, slab by slab. The LDS image is a heap block of exactly the plan's size, filled with a pattern before
 * every workgroup. The CPU suite (-m "not gpu") checks it against a numpy restatement, and the GPU suite holds the kernel to it.
 * It lives under tests/ and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../saprobe-alac_amd/csrc/alac_stack.h"

using namespace alacst;

extern "C" {

/* alacgpu_stack_create's check + alacgpu_stack_plan's numbers: info = {columns, tile_out, tile_in, tile_bins, lds_bytes,
 * w1_entries, w2_entries}, weights: kMaxWeights floats (or NULL). -> 0, or -2 where create is ALACGPU_E_ARG */
int stack_sim_plan(uint32_t bins, uint32_t order, uint32_t window, uint32_t left, uint32_t right, uint32_t stride, uint32_t* info,
                   float* weights) {
    const Config c{bins, order, window, left, right, stride, 0.0f};
    if (!info || !config_ok(c)) return -2;
    const Plan pl = plan_of(c);
    float w[kMaxWeights];
    uint32_t counts[2];
    const uint32_t n = make_weights(order, window, w, counts);
    info[0] = pl.cols;
    info[1] = pl.tile_out;
    info[2] = pl.tile_in;
    info[3] = pl.tile_bins;
    info[4] = pl.lds_floats * (uint32_t)sizeof(float);
    info[5] = counts[0];
    info[6] = counts[1];
    if (weights) memcpy(weights, w, n * sizeof(float));
    return 0;
}

/* The arguments of alacgpu_stack_create and alacgpu_stack_device with host pointers. -> 0, or -2 for what the entries reject. */
int stack_sim_run(uint32_t bins, uint32_t order, uint32_t window, uint32_t left, uint32_t right, uint32_t stride, float pad_value,
                  const float* in, uint64_t in_rs, uint64_t in_fs, uint64_t in_bs, uint64_t rows, uint64_t frames,
                  const int32_t* lengths, float* out, uint64_t out_rs, uint64_t out_fs, uint64_t out_bs, int32_t* out_lengths) {
    const Config c{bins, order, window, left, right, stride, pad_value};
    if (!config_ok(c)) return -2;
    if (rows == 0 || frames == 0) return 0;
    const Plan pl = plan_of(c);
    std::vector<float> w(kMaxWeights);
    uint32_t counts[2];
    w.resize(make_weights(order, window, w.data(), counts)); /* exactly the taps: a read beside them is the sanitizer's finding */
    Params p;
    if (!make_params(c, pl, in, in_rs, in_fs, in_bs, rows, frames, lengths, out, out_rs, out_fs, out_bs, out_lengths, w.data(), &p))
        return -2;
    std::vector<float> lds(pl.lds_floats);
    const auto each = [](auto&& phase) {
        for (uint32_t tid = 0; tid < kThreads; tid++) phase(tid);
    };
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.tiles; tile++) {
            const Tile t = make_tile(p, row, tile);
            memset(lds.data(), 0xA5, lds.size() * sizeof(float)); /* LDS holds whatever the last workgroup left */
            each([&](uint32_t tid) { put_length(p, t, tid); });
            for (uint32_t b0 = 0; b0 < p.bins; b0 += p.tile_bins) {
                if (t.gv) {
                    each([&](uint32_t tid) { stage_slab(p, t, b0, lds.data(), tid); });
                    if (p.order) each([&](uint32_t tid) { delta_slab(p, t, b0, lds.data(), tid); });
                }
                each([&](uint32_t tid) { store_slab(p, t, b0, lds.data(), tid); });
            }
        }
    return 0;
}

}  // extern "C"
