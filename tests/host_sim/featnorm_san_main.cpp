/*
 * featnorm_san_main.cpp — TEST-ONLY stand-alone program over featnorm_sim.cpp's functions, meant to be built with
 * -fsanitize=address,undefined and run on the CPU (tests/test_featnorm_host.py builds it plainly and runs it once): the bins 1,
 * 23, 80 and 129 at 2 * tile_frames + 3 frames, six rows with the lengths 0, 1, a middle value, frames, -5 and frames + 7, every
 * statistic with and without the affine step, both layouts, out of place and in place. Input, output and stats are heap blocks
 * of exactly the elements the pass may touch, and the LDS image is exactly the plan's size, so any access beside them is the
 * sanitizer's finding. Prints one line per pass with a sum of the outputs; exit status 0 when every pass ran, 1 otherwise.
 */
#include <cstdio>
#include <vector>

#include "featnorm_sim.cpp"

int main() {
    const uint32_t all_bins[] = {1, 23, 80, 129};
    int bad = 0;
    for (uint32_t bins : all_bins)
        for (uint32_t stat = 0; stat <= kMax; stat++)
            for (int layout = 0; layout < 2; layout++)
                for (int variant = 0; variant < 2; variant++) { /* 0: out of place, no affine; 1: in place, affine */
                    uint32_t info[2];
                    if (featnorm_sim_plan(bins, stat, 1e-20f, 8.0f, info) != 0) return 1;
                    const uint64_t rows = 6, frames = 2u * info[0] + 3u;
                    const int32_t lengths[6] = {0, 1, (int32_t)(frames + 1) / 2, (int32_t)frames, -5, (int32_t)frames + 7};
                    const uint64_t fs = layout ? 1u : bins, bs = layout ? frames : 1u, rs = frames * bins;
                    std::vector<float> in(rows * rs), out(rows * rs, -1.0f), stats(rows * 2u * bins, -1.0f), shift(bins), scale(bins);
                    uint32_t seed = 12345u + bins;
                    for (float& v : in) {
                        seed = seed * 1664525u + 1013904223u;
                        v = (float)(int32_t)(seed >> 8) * (1.0f / 1048576.0f) - 6.0f;
                    }
                    for (uint32_t b = 0; b < bins; b++) {
                        shift[b] = -4.0f + 0.01f * (float)b;
                        scale[b] = 0.25f + 0.001f * (float)b;
                    }
                    float* dst = variant ? in.data() : out.data();
                    const int rc = featnorm_sim_run(bins, stat, 1e-20f, 8.0f, -2.0f, variant ? shift.data() : nullptr,
                                                    variant ? scale.data() : nullptr, in.data(), rs, fs, bs, rows, frames, lengths, dst,
                                                    rs, fs, bs, stats.data());
                    double sum = 0.0;
                    for (uint64_t i = 0; i < rows * rs; i++) sum += dst[i];
                    printf("bins %u, stat %u, layout %d, variant %d, frames %llu, tile_frames %u -> %d, sum %.9g\n", bins, stat, layout,
                           variant, (unsigned long long)frames, info[0], rc, sum);
                    if (rc != 0) bad = 1;
                }
    return bad;
}
