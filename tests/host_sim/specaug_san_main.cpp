/*
 * specaug_san_main.cpp — TEST-ONLY stand-alone program over specaug_sim.cpp's functions, meant to be built with
 * -fsanitize=address,undefined and run on the CPU (tests/test_specaug_host.py builds it plainly and runs it once): five parameter
 * sets (nothing, masks only, a warp only, everything, the maxima) at the bins 1, 23, 80 and 129 and 3 * tile_out + 5 frames (the
 * maxima also at 530 frames, where a warp of 256 takes effect), seven rows with the lengths -3, 0, 1, 2 W, 2 W + 1, frames and
 * frames + 9, both layouts in and out, and in place where there is no warp. Input, output, lengths, ids and draws are heap blocks
 * of exactly the elements the pass may touch and the LDS block exactly the plan's size, so any access beside them is the
 * sanitizer's finding. Prints one line per pass with a sum of the outputs; exit status 0 when every pass ran, 1 otherwise.
 */
#include <cstdio>
#include <vector>

#include "specaug_sim.cpp"

int main() {
    const uint32_t sets[][6] = {/* freq_masks, freq_width (cut to the bins), time_masks, time_width, time_ratio_q16, warp */
                                {0, 0, 0, 0, 65536, 0}, {2, 10, 2, 20, 65536, 0}, {0, 0, 0, 0, 65536, 5}, {2, 10, 2, 20, 13107, 5},
                                {8, 4096, 16, 65535, 65536, 256}};
    const uint32_t all_bins[] = {1, 23, 80, 129};
    int bad = 0, passes = 0;
    for (const auto& s : sets)
        for (uint32_t bins : all_bins)
            for (int longer = 0; longer < 2; longer++) {
                if (longer && !(s[5] == 256u && bins == 23u)) continue;
                const uint32_t cfg[7] = {bins, s[0], s[1] < bins ? s[1] : bins, s[2], s[3], s[4], s[5]};
                uint32_t info[3];
                if (specaug_sim_plan(cfg, info) != 0) return 1;
                const uint64_t rows = 7, frames = longer ? 530u : 3u * info[1] + 5u, P = info[0];
                const int32_t lengths[7] = {-3, 0, 1, (int32_t)(2u * s[5]), (int32_t)(2u * s[5] + 1u), (int32_t)frames, (int32_t)frames + 9};
                const std::vector<int64_t> ids = {5, -1, 1ll << 40, 0, 7, 7, 123456789};
                std::vector<float> in(rows * frames * bins);
                uint32_t seed = 12345u + bins;
                for (float& v : in) {
                    seed = seed * 1664525u + 1013904223u;
                    v = (float)(int32_t)(seed >> 8) * (1.0f / 1048576.0f) - 6.0f;
                }
                for (int il = 0; il < 2; il++)
                    for (int ol = 0; ol < 3; ol++) { /* ol 2: in place */
                        if (ol == 2 && s[5] != 0u) continue;
                        std::vector<float> work(in), other(rows * frames * bins, -1.0f);
                        std::vector<int32_t> draws(rows * P, -1);
                        const int lay = ol == 2 ? il : ol;
                        float* out = ol == 2 ? work.data() : other.data();
                        const int rc = specaug_sim_run(cfg, -7.0f, -2.0f, work.data(), frames * bins, il ? 1u : bins, il ? frames : 1u, rows,
                                                       frames, lengths, 0x9E3779B97F4A7C15ull, 3u, il ? ids.data() : nullptr, out,
                                                       frames * bins, lay ? 1u : bins, lay ? frames : 1u, draws.data());
                        double sum = 0.0;
                        for (uint64_t i = 0; i < rows * frames * bins; i++) sum += out[i];
                        long total = 0;
                        for (int32_t d : draws) total += d;
                        printf("bins %u, masks %u x %u + %u x %u, ratio %u, warp %u, layouts %d / %d, frames %llu, tile %u -> %d, sum %.9g, "
                               "draws %ld\n", bins, cfg[1], cfg[2], cfg[3], cfg[4], cfg[5], cfg[6], il, ol, (unsigned long long)frames,
                               info[1], rc, sum, total);
                        passes++;
                        if (rc != 0) bad = 1;
                    }
            }
    printf("%d passes\n", passes);
    return bad;
}
