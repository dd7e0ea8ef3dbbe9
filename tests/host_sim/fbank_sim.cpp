/*
 * fbank_sim.cpp — TEST-ONLY host build of the Kaldi feature pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_fbank.h (the text the gfx950 kernel of k_fbank.hip is built from) with g++, contraction
 * off, and runs it the way k_fbank.hip launches it: for every tile of every row the phases of alacfb::tile_phase, each for work
 * items 0..255, a barrier between two phases. The CPU suite (-m "not gpu") checks it against a numpy restatement, and the GPU
 * suite holds the kernel to it bit for bit. It lives under tests/ and is never linked into libalacgpu.so.
 *
 * With -DFBANK_SIM_MAIN it is a program of its own that runs a few parameter sets over guarded inputs and exact-size outputs:
 * the build to run under -fsanitize=address,undefined (g++ -DFBANK_SIM_MAIN -ffp-contract=off -fsanitize=address,undefined).
 */
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_fbank.h"

using namespace alacfb;

namespace {
/* cfg = {sample_rate, frame_length, frame_shift, round_to_power_of_two, num_mel_bins, num_ceps, snip_edges, remove_dc_offset,
 * window_type, use_log_fbank, use_energy, raw_energy, htk_compat, use_power, log_energy, layout};
 * dbl = {preemphasis, blackman_coeff, low_freq, high_freq, energy_floor, scale, cepstral_lifter, dither, vtln_warp} */
Config config_of(const uint32_t* cfg, const double* dbl) {
    Config c;
    c.sample_rate = cfg[0];
    c.frame_length = cfg[1];
    c.frame_shift = cfg[2];
    c.round_to_power_of_two = cfg[3];
    c.num_mel_bins = cfg[4];
    c.num_ceps = cfg[5];
    c.snip_edges = cfg[6];
    c.remove_dc_offset = cfg[7];
    c.window_type = cfg[8];
    c.use_log_fbank = cfg[9];
    c.use_energy = cfg[10];
    c.raw_energy = cfg[11];
    c.htk_compat = cfg[12];
    c.use_power = cfg[13];
    c.log_energy = cfg[14];
    c.layout = cfg[15];
    c.preemphasis = dbl[0];
    c.blackman_coeff = dbl[1];
    c.low_freq = dbl[2];
    c.high_freq = dbl[3];
    c.energy_floor = dbl[4];
    c.scale = dbl[5];
    c.cepstral_lifter = dbl[6];
    c.dither = dbl[7];
    c.vtln_warp = dbl[8];
    return c;
}
}  // namespace

extern "C" {

/* alacgpu_fbank_create + alacgpu_fbank_plan: info = the ten numbers of alacgpu_fbank_info; the table pointers may be NULL.
 * -> 0, or -2 where the entries return ALACGPU_E_ARG. */
int fbank_sim_plan(const uint32_t* cfg, const double* dbl, uint32_t* info, float* basis_out, uint64_t basis_cap, float* fb_out,
                   uint64_t fb_cap, int32_t* first_out, uint64_t first_cap, float* dct_out, uint64_t dct_cap, float* lifter_out,
                   uint64_t lifter_cap) {
    Plan pl;
    if (!cfg || !dbl || !info || !make_plan(config_of(cfg, dbl), &pl)) return -2;
    if ((basis_out && basis_cap < pl.basis.size()) || (fb_out && fb_cap < pl.fbw.size()) || (first_out && first_cap < pl.first.size()) ||
        (dct_out && dct_cap < pl.dct.size()) || (lifter_out && lifter_cap < pl.lifter.size()))
        return -2;
    const uint32_t numbers[10] = {pl.W, pl.hop, pl.N, pl.K, pl.n_mels, pl.taps, pl.num_ceps, pl.cols, pl.tile_frames, pl.lds_floats * 4u};
    memcpy(info, numbers, sizeof(numbers));
    if (basis_out) memcpy(basis_out, pl.basis.data(), pl.basis.size() * sizeof(float));
    if (fb_out) memcpy(fb_out, pl.fbw.data(), pl.fbw.size() * sizeof(float));
    if (first_out) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    if (dct_out && !pl.dct.empty()) memcpy(dct_out, pl.dct.data(), pl.dct.size() * sizeof(float));
    if (lifter_out && !pl.lifter.empty()) memcpy(lifter_out, pl.lifter.data(), pl.lifter.size() * sizeof(float));
    return 0;
}

/* alacgpu_fbank_out_frames; 0 where there is no plan or no frame */
uint64_t fbank_sim_out_frames(const uint32_t* cfg, const double* dbl, uint64_t in_frames) {
    Plan pl;
    if (!make_plan(config_of(cfg, dbl), &pl) || in_frames > ((uint64_t)1 << 61)) return 0;
    return out_frames_of(pl.W, pl.hop, pl.cfg.snip_edges, in_frames);
}

/* The arguments of alacgpu_fbank_device with host pointers. -> 0, or -2 for what the entries reject. guard != 0: the input,
 * (rows - 1) * in_stride + in_frames elements, is copied so that it ENDS at an inaccessible page, and the pass reads the copy:
 * a read behind the last row's samples is fatal. */
int fbank_sim_run(const uint32_t* cfg, const double* dbl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames,
                  float* out, uint64_t out_row_stride, uint64_t out_inner_stride, int guard) {
    Plan pl;
    if (!make_plan(config_of(cfg, dbl), &pl)) return -2;
    if (in_frames > ((uint64_t)1 << 61)) return rows ? -2 : 0;
    if (rows == 0 || out_frames_of(pl.W, pl.hop, pl.cfg.snip_edges, in_frames) == 0) return 0;
    Params p;
    if (!make_params(pl, in, in_stride, rows, in_frames, out, out_row_stride, out_inner_stride, pl.bt.data(), pl.fbw.data(),
                     pl.first.data(), pl.dct.data(), pl.lifter.data(), &p))
        return -2;

    uint8_t* region = nullptr;
    size_t region_len = 0;
    if (guard) {
        const size_t bytes = (size_t)((rows - 1) * in_stride + in_frames) * sizeof(float);
        const size_t page = (size_t)sysconf(_SC_PAGESIZE);
        region_len = (bytes + page - 1) / page * page + page;
        region = (uint8_t*)mmap(nullptr, region_len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (region == MAP_FAILED) return -3;
        uint8_t* copy = region + region_len - page - bytes;
        memcpy(copy, in, bytes);
        mprotect(region + region_len - page, page, PROT_NONE);
        p.m.in = (const float*)copy;
    }
    alignas(16) static thread_local float lds[kLdsFloats];
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.m.tiles_per_row; tile++) {
            const Tile t = make_tile(p, row, tile);
            if (t.count == 0) continue;
            memset(lds, 0xA5, sizeof(lds)); /* LDS holds whatever the last workgroup left */
            for (uint32_t phase = 0; phase < 5u; phase++)
                for (uint32_t tid = 0; tid < kThreads; tid++) tile_phase(p, t, lds, phase, tid);
        }
    if (region) munmap(region, region_len);
    return 0;
}

uint32_t fbank_sim_lds_floats(void) { return kLdsFloats; }

}  // extern "C"

#ifdef FBANK_SIM_MAIN
#include <cstdlib>
#include <vector>

/* A few parameter sets (every branch of the staging, both layouts, energy, MFCC), each over rows 3 at F = tile_frames + 1 with
 * the input ending at a guard page and the output exactly as large as what is written: for builds with a sanitizer. */
int main() {
    struct Case {
        uint32_t w[16];
        double d[9];
    };
    const Case cases[] = {
        {{8000, 10, 4, 1, 23, 0, 1, 1, 2, 1, 0, 1, 0, 1, 1, 0}, {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}},
        {{8000, 9, 5, 1, 23, 0, 0, 1, 2, 1, 1, 1, 0, 1, 1, 0}, {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}},
        {{8000, 16, 37, 1, 23, 0, 0, 1, 0, 1, 1, 1, 1, 1, 1, 1}, {0.97, 0.42, 20, 0, 0.0, 32768.0, 22, 0, 1}},
        {{8000, 7, 3, 0, 5, 0, 1, 0, 4, 0, 0, 1, 0, 1, 1, 1}, {0.0, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}},
        {{8000, 50, 20, 1, 23, 13, 1, 1, 2, 1, 1, 1, 1, 1, 1, 0}, {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}},
        {{16000, 400, 160, 1, 80, 0, 1, 1, 2, 1, 0, 1, 0, 1, 1, 0}, {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}},
        {{16000, 64, 16, 1, 2048, 0, 1, 1, 2, 1, 0, 1, 0, 1, 1, 0}, {0.97, 0.42, 20, 0, 1.0, 1.0, 22, 0, 1}},
    };
    int bad = 0;
    for (const Case& c : cases) {
        uint32_t info[10];
        if (fbank_sim_plan(c.w, c.d, info, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0) != 0) {
            printf("no plan\n");
            return 1;
        }
        const uint32_t W = info[0], h = info[1], cols = info[7], tf = info[8];
        const uint64_t rows = 3;
        uint64_t T = W + (uint64_t)tf * h;
        while (fbank_sim_out_frames(c.w, c.d, T) < tf + 1u) T++;
        const uint64_t F = fbank_sim_out_frames(c.w, c.d, T);
        std::vector<float> in(rows * T);
        uint32_t s = 12345u;
        for (float& v : in) {
            s = s * 1664525u + 1013904223u;
            v = (float)((int32_t)(s >> 8) % 32768 - 16384) * (1.0f / 16384.0f);
        }
        const bool bins = c.w[15] == 1u;
        const uint64_t inner = bins ? F : cols, row_stride = F * cols;
        float* out = (float*)malloc(rows * row_stride * sizeof(float)); /* exactly what is written: one element more is caught */
        const int rc = fbank_sim_run(c.w, c.d, in.data(), T, rows, T, out, row_stride, inner, 1);
        double sum = 0.0;
        for (uint64_t i = 0; i < rows * row_stride; i++) sum += out[i];
        printf("W %u h %u cols %u tile_frames %u T %llu F %llu rc %d sum %g\n", W, h, cols, tf, (unsigned long long)T,
               (unsigned long long)F, rc, sum);
        bad |= rc;
        free(out);
    }
    return bad ? 1 : 0;
}
#endif
