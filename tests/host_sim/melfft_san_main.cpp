/*
 * melfft_san_main.cpp — TEST-ONLY stand-alone program over melfft_sim.cpp's functions, meant to be built with
 * -fsanitize=address,undefined and run on the CPU (tests/test_melfft_host.py does both): three parameter sets, each with the
 * input ending at the last element of its heap buffer and again at an inaccessible page, the LDS image exactly the plan's size
 * on the heap, the output exactly [rows][bins][F]. Prints one line per pass with a sum of the outputs; exit status 0 when
 * every pass ran, 1 otherwise. Any finding is the sanitizer's own abort.
 */
#include <cstdio>
#include <vector>

#include "melfft_sim.cpp"

namespace {
struct Case {
    const char* name;
    uint32_t cfg[9]; /* sample_rate, n_fft, win_length, hop_length, n_mels, center, norm, mel_scale, log */
    double dbl[3];   /* f_min, f_max, floor */
    uint64_t rows, frames;
};

uint64_t length_for(const Case& c) {
    const uint64_t N = c.cfg[1], h = c.cfg[3];
    if (c.cfg[5]) return (c.frames - 1) * h > N / 2 + 1 ? (c.frames - 1) * h : N / 2 + 1;
    return N + (c.frames - 1) * h;
}
}  // namespace

int main() {
    const Case cases[] = {
        {"n30 5x3, 5 mels, 70 frames", {8000, 30, 30, 11, 5, 1, 0, 1, 0}, {0.0, 4000.0, 1e-10}, 3, 70},
        {"whisper, 21 frames, log10", {16000, 400, 400, 160, 80, 1, 1, 2, 2}, {0.0, 8000.0, 1e-10}, 2, 21},
        {"n2048 hop 5000, power only, not centred, 6 frames", {48000, 2048, 2048, 5000, 0, 0, 0, 0, 0}, {0.0, 24000.0, 1e-10}, 2, 6},
    };
    int bad = 0;
    for (const Case& c : cases) {
        const uint64_t T = length_for(c);
        const uint64_t F = alacmel::out_frames_of(c.cfg[1], c.cfg[3], c.cfg[5], T);
        const uint64_t bins = c.cfg[4] ? c.cfg[4] : c.cfg[1] / 2u + 1u;
        std::vector<float> in(c.rows * T), out(c.rows * bins * F, -1.0f);
        uint32_t seed = 12345u;
        for (float& v : in) {
            seed = seed * 1664525u + 1013904223u;
            v = (float)(int32_t)(seed >> 8) * (1.0f / 8388608.0f) - 1.0f;
        }
        for (int guard = 0; guard < 2; guard++) {
            const int rc = melfft_sim_run(c.cfg, c.dbl, in.data(), T, c.rows, T, out.data(), bins * F, F, guard);
            double sum = 0.0;
            for (float v : out) sum += v;
            printf("%s: T %llu, F %llu, guard %d -> %d, sum %.9g\n", c.name, (unsigned long long)T, (unsigned long long)F, guard, rc, sum);
            if (rc != 0 || F != c.frames) bad = 1;
        }
    }
    return bad;
}
