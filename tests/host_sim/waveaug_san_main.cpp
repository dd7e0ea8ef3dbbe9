/*
 * waveaug_san_main.cpp — TEST-ONLY stand-alone program over waveaug_sim.cpp's functions, meant to be built with
 * -fsanitize=address,undefined and run on the CPU (tests/test_waveaug_host.py builds it plainly and runs it once): five parameter
 * sets (nothing, gain only, noise only, dither only, everything with clamp) at the sample counts 1, 255, 257, 4096, 4097 and 2 *
 * 4096 + 3, six rows with the lengths -2, 0, 1, T - 1, T and T + 9, banks of 0 and 3 clips of the lengths 0, 1, 2, 257, 4097 and 9000,
 * every base offset of input, output and bank, in place and not. Three switches run independently of the bank: a stats block or
 * none (so the handle's own stats behind the partials, and stats without a bank, both occur), `bare` (no lengths, no ids, no draws;
 * so draws without stats occur, and the apply kernel alone with and without them), in place. Then two passes more: two rows of 257
 * chunks + 3 samples (the finish kernel's second block of partials), and clips of 100 samples under rows of 2 * 4096 + 3 (the walk
 * of a clip shorter than a chunk). Input, output, bank, lengths, ids, draws and stats are heap blocks of exactly the elements the
 * pass may touch and the LDS and scratch blocks exactly the plan's sizes, so any access beside them is the sanitizer's finding.
 * Prints one line per pass with a sum of the outputs; exit status 0 when every pass ran, 1 otherwise.
 */
#include <cstdio>
#include <vector>

#include "waveaug_sim.cpp"

static const int32_t sets[][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, -1536, 768, 0, 0}, {1280, 5120, 0, 0, 65536, 0}, {0, 0, 0, 0, 0, 0},
                                  {-768, 3847, -1537, 768, 52429, 1}};
static const float dithers[] = {0.0f, 0.0f, 0.0f, 0.1f, 0.01f};

/* One pass over `rows` rows of T samples with the lengths -2, 0, 1, T - 1, T, T + 9 (the last `rows` of them), a bank of the three
 * clips `cl` (null: none) on a stride of Tn. -> waveaug_sim_run's return code */
static int one_pass(int si, uint64_t T, uint64_t rows, const int32_t* cl, uint64_t Tn, int k, bool in_place, bool bare, bool with_stats) {
    const uint64_t N = cl ? 3 : 0;
    const int32_t all_lengths[6] = {-2, 0, 1, (int32_t)T - 1, (int32_t)T, (int32_t)T + 9};
    const int32_t* lengths = all_lengths + (6u - rows);
    const std::vector<int64_t> ids = {5, -1, 1ll << 40, 0, 7, 123456789};
    const uint64_t lead = (uint64_t)k % 4u, gap = (uint64_t)(k / 4) % 3u;
    /* exactly lead + (rows - 1) * (T + gap) + T elements; vector storage is 16-byte aligned */
    std::vector<float> in(lead + (rows - 1u) * (T + gap) + T);
    std::vector<float> other(in_place ? 0u : (lead + 1u) % 4u + (rows - 1u) * (T + gap) + T, -1.0f);
    uint32_t seed = 12345u + (uint32_t)T;
    for (float& v : in) {
        seed = seed * 1664525u + 1013904223u;
        v = (float)(int32_t)(seed >> 8) * (1.0f / 16777216.0f) - 0.5f;
    }
    std::vector<float> bank;
    std::vector<int32_t> nl;
    if (N) {
        nl.assign(cl, cl + 3);
        /* clip j holds exactly its valid samples: the stride is the longest clip's, the last row is cut short */
        bank.resize(lead + 2u * Tn + (uint64_t)cl[2]);
        for (float& v : bank) {
            seed = seed * 1664525u + 1013904223u;
            v = (float)(int32_t)(seed >> 8) * (1.0f / 67108864.0f) - 0.125f;
        }
    }
    std::vector<int32_t> draws(rows * 5u, -1);
    std::vector<float> stats(with_stats ? rows * 4u : 0u, -1.0f);
    float* out = in_place ? in.data() + lead : other.data() + (lead + 1u) % 4u;
    const int rc = waveaug_sim_run(sets[si], dithers[si], -2.0f, in.data() + lead, T + gap, rows, T, bare ? nullptr : lengths,
                                   N ? bank.data() + lead : nullptr, Tn, N, N ? (uint64_t)nl[2] : 0u, N ? nl.data() : nullptr,
                                   0x9E3779B97F4A7C15ull, 3u, bare ? nullptr : ids.data(), out, T + gap, bare ? nullptr : draws.data(),
                                   with_stats ? stats.data() : nullptr);
    double sum = 0.0;
    for (uint64_t r = 0; r < rows; r++)
        for (uint64_t t = 0; t < T; t++) sum += out[r * (T + gap) + t];
    long total = 0;
    for (int32_t d : draws) total += d;
    printf("set %d, T %llu, rows %llu, bank %d (%d, %d, %d), lead %llu, gap %llu, in place %d, bare %d, stats %d -> %d, sum %.9g, draws %ld\n",
           si, (unsigned long long)T, (unsigned long long)rows, (int)N, cl ? cl[0] : 0, cl ? cl[1] : 0, cl ? cl[2] : 0,
           (unsigned long long)lead, (unsigned long long)gap, (int)in_place, (int)bare, (int)with_stats, rc, sum, total);
    return rc;
}

int main() {
    const uint64_t all_T[] = {1, 255, 257, 4096, 4097, 2 * 4096 + 3};
    const int32_t clip_lengths[2][3] = {{0, 1, 9000}, {2, 257, 4097}};
    int bad = 0, passes = 0, k = 0, seen[2][2][2] = {};
    for (int si = 0; si < 5; si++)
        for (uint64_t T : all_T)
            for (int banked = 0; banked < 3; banked++) { /* 0: no bank; 1, 2: three clips */
                /* banked is k % 3; the three switches have the periods 2, 5 and 4 x 3 in k, so each meets every bank */
                const bool in_place = k % 2 == 1, bare = k % 5 == 4, with_stats = (k / 3) % 4 < 2 ? banked != 1 : banked == 1;
                seen[banked != 0][with_stats][!bare]++;
                if (one_pass(si, T, 6, banked ? clip_lengths[banked - 1] : nullptr, 9000, k, in_place, bare, with_stats)) bad = 1;
                k++;
                passes++;
            }
    for (int b = 0; b < 2; b++)
        for (int s = 0; s < 2; s++)
            for (int d = 0; d < 2; d++) {
                printf("bank %d, stats %d, draws %d: %d of the passes above\n", b, s, d, seen[b][s][d]);
                if (!seen[b][s][d]) bad = 1;
            }
    /* a row of more than 256 chunks: the finish kernel's second block; with the handle's own stats block */
    const int32_t long_clips[3] = {5000, 257, 5000};
    if (one_pass(4, 257u * 4096u + 3u, 2, long_clips, 5000, 1, false, false, false)) bad = 1;
    /* clips shorter than a chunk, walked in steps of 256 mod 100 */
    const int32_t short_clips[3] = {100, 100, 100};
    if (one_pass(2, 2u * 4096u + 3u, 6, short_clips, 100, 2, true, false, true)) bad = 1;
    passes += 2;
    printf("%d passes\n", passes);
    return bad;
}
