/*
 * stack_san_main.cpp — TEST-ONLY stand-alone program over stack_sim.cpp's functions, meant to be built with
 * -fsanitize=address,undefined and run on the CPU (tests/test_stack_host.py builds it plainly and runs it once): seven parameter
 * sets (copy, add-deltas, deltas with context, LFR 7/6, deltas under LFR, the widest window and context at stride 64, and one
 * whose bins go in slabs) at up to four bin counts and 2 * tile_in + 3 frames, six rows with the lengths 0, 1, a middle value,
 * frames, -5 and frames + 7, both layouts in and out. Input, output and lengths are heap blocks of exactly the elements the pass
 * may touch, the weights exactly the taps and the LDS image exactly the plan's size, so any access beside them is the
 * sanitizer's finding. Prints one line per pass with a sum of the outputs; exit status 0 when every pass ran, 1 otherwise.
 */
#include <cstdio>
#include <vector>

#include "stack_sim.cpp"

int main() {
    const uint32_t sets[][6] = {/* order, window, left, right, stride, the largest bins */
                                {0, 0, 0, 0, 1, 129}, {2, 2, 0, 0, 1, 129}, {2, 3, 1, 1, 1, 129}, {0, 0, 3, 3, 6, 129},
                                {2, 2, 3, 3, 6, 129}, {1, 8, 16, 16, 64, 23}, {2, 8, 0, 0, 1, 700}};
    const uint32_t all_bins[] = {1, 23, 80, 129, 700};
    int bad = 0, passes = 0;
    for (const auto& s : sets)
        for (uint32_t bins : all_bins) {
            if (bins > s[5] || (s[5] == 700u && bins != 700u)) continue;
            uint32_t info[7];
            if (stack_sim_plan(bins, s[0], s[1], s[2], s[3], s[4], info, nullptr) != 0) return 1;
            const uint64_t rows = 6, frames = 2u * info[2] + 3u, G = (frames + s[4] - 1u) / s[4], D = info[0];
            const int32_t lengths[6] = {0, 1, (int32_t)(frames + 1) / 2, (int32_t)frames, -5, (int32_t)frames + 7};
            std::vector<float> in(rows * frames * bins);
            uint32_t seed = 12345u + bins;
            for (float& v : in) {
                seed = seed * 1664525u + 1013904223u;
                v = (float)(int32_t)(seed >> 8) * (1.0f / 1048576.0f) - 6.0f;
            }
            for (int il = 0; il < 2; il++)
                for (int ol = 0; ol < 2; ol++) {
                    std::vector<float> out(rows * G * D, -1.0f);
                    std::vector<int32_t> out_lengths(rows, -1);
                    const int rc = stack_sim_run(bins, s[0], s[1], s[2], s[3], s[4], -2.0f, in.data(), frames * bins, il ? 1u : bins,
                                                 il ? frames : 1u, rows, frames, lengths, out.data(), G * D, ol ? 1u : D, ol ? G : 1u,
                                                 out_lengths.data());
                    double sum = 0.0;
                    for (float v : out) sum += v;
                    long total = 0;
                    for (int32_t m : out_lengths) total += m;
                    printf("bins %u, order %u, window %u, context %u + %u, stride %u, layouts %d / %d, frames %llu, tile %u x %u -> %d, "
                           "sum %.9g, lengths %ld\n", bins, s[0], s[1], s[2], s[3], s[4], il, ol, (unsigned long long)frames, info[1],
                           info[3], rc, sum, total);
                    passes++;
                    if (rc != 0) bad = 1;
                }
        }
    printf("%d passes\n", passes);
    return bad;
}
