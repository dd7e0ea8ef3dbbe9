/*
 * specaug_sim.cpp — TEST-ONLY host build of the SpecAugment pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_specaug.h (the text the gfx950 kernel of k_specaug.hip is built from) with g++, contraction
 * off, and runs it the way k_specaug.hip launches it: for every workgroup (row, tile) each phase for work items 0..255 with the
 * barriers between them. The LDS block is a heap block of exactly the plan's size, filled with a pattern before every workgroup.
 * The CPU suite (-m "not gpu") checks it against a numpy restatement, and the GPU suite holds the kernel to it. It lives under
 * tests/ and is never linked into libalacgpu.so.
 */
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../saprobe-alac_amd/csrc/alac_specaug.h"

using namespace alacsa;

extern "C" {

/* cfg = {bins, freq_masks, freq_width, time_masks, time_width, time_ratio_q16, warp} */
static Config config_of(const uint32_t* cfg, float mask_value, float pad_value) {
    return Config{cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], cfg[6], mask_value, pad_value};
}

/* one Philox4x32-10 block: counter[4], key[2] -> out[4] */
void specaug_sim_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
    philox4x32_10(c, key[0], key[1]);
    memcpy(out, c, sizeof(c));
}

/* alacgpu_specaug_create's check + alacgpu_specaug_plan's numbers: info = {draws, tile_out, lds_bytes}.
 * -> 0, or -2 where create is ALACGPU_E_ARG */
int specaug_sim_plan(const uint32_t* cfg, uint32_t* info) {
    const Config c = config_of(cfg, 0.0f, 0.0f);
    if (!info || !config_ok(c)) return -2;
    const Plan pl = plan_of(c);
    info[0] = pl.draws;
    info[1] = pl.tile_out;
    info[2] = pl.lds_words * 4u;
    return 0;
}

/* The arguments of alacgpu_specaug_create and alacgpu_specaug_device with host pointers. -> 0, or -2 for what the entries reject. */
int specaug_sim_run(const uint32_t* cfg, float mask_value, float pad_value, const float* in, uint64_t in_rs, uint64_t in_fs,
                    uint64_t in_bs, uint64_t rows, uint64_t frames, const int32_t* lengths, uint64_t seed, uint64_t row_base,
                    const int64_t* ids, float* out, uint64_t out_rs, uint64_t out_fs, uint64_t out_bs, int32_t* draws) {
    const Config c = config_of(cfg, mask_value, pad_value);
    if (!config_ok(c)) return -2;
    if (rows == 0 || frames == 0) return 0;
    const Plan pl = plan_of(c);
    Params p;
    if (!make_params(c, pl, in, in_rs, in_fs, in_bs, rows, frames, lengths, seed, row_base, ids, out, out_rs, out_fs, out_bs, draws, &p))
        return -2;
    std::vector<float> lds(pl.lds_words);
    const Lds l = carve(p, lds.data());
    const auto each = [](auto&& phase) {
        for (uint32_t tid = 0; tid < kThreads; tid++) phase(tid);
    };
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.tiles; tile++) {
            const Tile t = make_tile(p, row, tile);
            memset(lds.data(), 0xA5, lds.size() * sizeof(float)); /* LDS holds whatever the last workgroup left */
            each([&](uint32_t tid) { resolve_draws(p, t, l.draws, tid); });
            each([&](uint32_t tid) {
                frame_plan(p, t, l, tid);
                bin_plan(p, l, tid);
            });
            each([&](uint32_t tid) { build_image(p, t, l, tid); });
            each([&](uint32_t tid) { store_image(p, t, l, tid); });
        }
    return 0;
}

}  // extern "C"
