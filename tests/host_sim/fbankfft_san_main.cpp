/*
 * fbankfft_san_main.cpp — TEST-ONLY stand-alone program over fbankfft_sim.cpp's functions, meant to be built with
 * -fsanitize=address,undefined and run on the CPU (tests/test_fbankfft_host.py builds it plainly and runs it once): three
 * parameter sets (W odd and below N; the ASR front end; W = N = 2048 with one frame in the transform buffer), each with the input
 * ending at the last element of its heap buffer and again at an inaccessible page, the LDS image exactly the plan's size on the
 * heap, the output exactly what is written. Prints one line per pass with a sum of the outputs; exit status 0 when every pass
 * ran, 1 otherwise. Any finding is the sanitizer's own abort.
 */
#include <cstdio>
#include <vector>

#include "fbankfft_sim.cpp"

namespace {
struct Case {
    const char* name;
    uint32_t w[16];
    double d[9];
    uint64_t rows, frames;
    uint32_t batch;
};
}  // namespace

int main() {
    const Case cases[] = {
        {"W 9 in N 16, reflected, energy, 66 frames", {8000, 9, 5, 1, 23, 0, 0, 1, 2, 1, 1, 1, 0, 1, 1, 0},
         {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}, 3, 66, 64},
        {"asr W 400 N 512, 80 bins, layout bins, 17 frames", {16000, 400, 160, 1, 80, 0, 1, 1, 2, 1, 0, 1, 0, 1, 1, 1},
         {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}, 2, 17, 16},
        {"full W = N = 2048, MFCC 13 with energy, 6 frames", {48000, 2048, 2048, 0, 23, 13, 1, 1, 2, 1, 1, 1, 0, 1, 1, 0},
         {0.97, 0.42, 20, 0, 1.0, 32768.0, 22, 0, 1}, 2, 6, 1},
    };
    int bad = 0;
    for (const Case& c : cases) {
        uint32_t info[33];
        if (fbankfft_sim_plan(c.w, c.d, info, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0) != 0) {
            printf("%s: no plan\n", c.name);
            return 1;
        }
        const uint64_t W = info[0], h = info[1], cols = info[7];
        const bool snip = c.w[6] != 0u;
        uint64_t T = W;
        while (alacfb::out_frames_of((uint32_t)W, (uint32_t)h, snip, T) < c.frames) T++;
        const uint64_t F = alacfb::out_frames_of((uint32_t)W, (uint32_t)h, snip, T);
        std::vector<float> in(c.rows * T), out(c.rows * cols * F, -1.0f);
        uint32_t seed = 12345u;
        for (float& v : in) {
            seed = seed * 1664525u + 1013904223u;
            v = (float)(int32_t)(seed >> 8) * (1.0f / 8388608.0f) - 0.75f;
        }
        const uint64_t inner = c.w[15] == 1u ? F : cols;
        for (int guard = 0; guard < 2; guard++) {
            const int rc = fbankfft_sim_run(c.w, c.d, in.data(), T, c.rows, T, out.data(), cols * F, inner, guard);
            double sum = 0.0;
            for (float v : out) sum += v;
            printf("%s: T %llu, F %llu, tile_frames %u, batch %u, guard %d -> %d, sum %.9g\n", c.name, (unsigned long long)T,
                   (unsigned long long)F, info[8], info[13], guard, rc, sum);
            if (rc != 0 || F != c.frames || info[13] != c.batch) bad = 1;
        }
    }
    return bad;
}
