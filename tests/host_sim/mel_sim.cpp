/*
 * mel_sim.cpp — TEST-ONLY host build of the spectrogram pass.
 *
 * Compiles saprobe-alac_amd/csrc/alac_mel.h (the text the gfx950 kernel of k_mel.hip is built from) with g++, contraction off,
 * and runs it the way k_mel.hip launches it: for every tile of every row the staging phase for work items 0..255, the barrier,
 * the DFT for work items 0..255, the barrier, the mel chains (or the log over the power tile), the barrier, and the store
 * phase. The CPU suite (-m "not gpu") checks it against a numpy restatement, and the GPU suite holds the kernel to it bit for
 * bit. It lives under tests/ and is never linked into libalacgpu.so.
 */
#include <sys/mman.h>
#include <unistd.h>

#include <cstdint>
#include <cstring>

#include "../../saprobe-alac_amd/csrc/alac_mel.h"

using namespace alacmel;

namespace {
/* cfg = {sample_rate, n_fft, win_length, hop_length, n_mels, center, norm, mel_scale, log}; dbl = {f_min, f_max, floor} */
Config config_of(const uint32_t* cfg, const double* dbl) {
    Config c;
    c.sample_rate = cfg[0];
    c.n_fft = cfg[1];
    c.win_length = cfg[2];
    c.hop_length = cfg[3];
    c.n_mels = cfg[4];
    c.center = cfg[5];
    c.norm = cfg[6];
    c.mel_scale = cfg[7];
    c.log = cfg[8];
    c.f_min = dbl[0];
    c.f_max = dbl[1];
    c.floor = dbl[2];
    return c;
}
}  // namespace

extern "C" {

/* alacgpu_mel_create + alacgpu_mel_plan: info = {n_fft, win_length, hop_length, n_freqs, n_mels, taps, bins, tile_frames,
 * lds_bytes}; the table pointers may be NULL. -> 0, or -2 where the entries return ALACGPU_E_ARG. */
int mel_sim_plan(const uint32_t* cfg, const double* dbl, uint32_t* info, float* basis_out, uint64_t basis_cap, float* fb_out,
                 uint64_t fb_cap, int32_t* first_out, uint64_t first_cap) {
    Plan pl;
    if (!cfg || !dbl || !info || !make_plan(config_of(cfg, dbl), &pl)) return -2;
    if ((basis_out && basis_cap < pl.basis.size()) || (fb_out && fb_cap < pl.fbw.size()) || (first_out && first_cap < pl.first.size()))
        return -2;
    const uint32_t numbers[9] = {pl.N, pl.W, pl.hop, pl.K, pl.n_mels, pl.n_mels ? pl.taps : 0u, pl.bins, pl.tile_frames, pl.lds_floats * 4u};
    memcpy(info, numbers, sizeof(numbers));
    if (basis_out) memcpy(basis_out, pl.basis.data(), pl.basis.size() * sizeof(float));
    if (fb_out && !pl.fbw.empty()) memcpy(fb_out, pl.fbw.data(), pl.fbw.size() * sizeof(float));
    if (first_out && !pl.first.empty()) memcpy(first_out, pl.first.data(), pl.first.size() * sizeof(int32_t));
    return 0;
}

/* alacgpu_mel_out_frames; 0 where there is no plan or no frame */
uint64_t mel_sim_out_frames(const uint32_t* cfg, const double* dbl, uint64_t in_frames) {
    Plan pl;
    if (!make_plan(config_of(cfg, dbl), &pl) || in_frames > ((uint64_t)1 << 61)) return 0;
    return out_frames_of(pl.N, pl.hop, pl.cfg.center, in_frames);
}

/* The arguments of alacgpu_mel_device with host pointers. -> 0, or -2 for what the entries reject. guard != 0: the input,
 * (rows - 1) * in_stride + in_frames elements, is copied so that it ENDS at an inaccessible page, and the pass reads the copy:
 * a read behind the last row's samples is fatal. */
int mel_sim_run(const uint32_t* cfg, const double* dbl, const float* in, uint64_t in_stride, uint64_t rows, uint64_t in_frames,
                float* out, uint64_t out_row_stride, uint64_t out_bin_stride, int guard) {
    Plan pl;
    if (!make_plan(config_of(cfg, dbl), &pl)) return -2;
    if (in_frames > ((uint64_t)1 << 61)) return rows ? -2 : 0;
    if (rows == 0 || out_frames_of(pl.N, pl.hop, pl.cfg.center, in_frames) == 0) return 0;
    Params p;
    if (!make_params(pl, in, in_stride, rows, in_frames, out, out_row_stride, out_bin_stride, pl.bt.data(), pl.fbw.data(),
                     pl.first.data(), &p))
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
        p.in = (const float*)copy;
    }
    alignas(16) static thread_local float lds[kLdsFloats];
    float* ptile = lds + p.a_floats;
    for (uint64_t row = 0; row < rows; row++)
        for (uint64_t tile = 0; tile < p.tiles_per_row; tile++) {
            const Tile t = make_tile(p, row, tile);
            if (t.count == 0) continue;
            memset(lds, 0xA5, sizeof(lds)); /* LDS holds whatever the last workgroup left */
            for (uint32_t tid = 0; tid < kThreads; tid++) stage_tile(p, t, lds, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) dft_tile(p, t, lds, ptile, tid);
            for (uint32_t tid = 0; tid < kThreads; tid++) {
                if (p.n_mels) mel_tile(p, ptile, lds, tid);
                else log_tile(p, ptile, tid);
            }
            for (uint32_t tid = 0; tid < kThreads; tid++) {
                if (p.n_mels) store_tile(p, t, lds, p.tile_frames, 1u, tid);
                else store_tile(p, t, ptile, 1u, p.KP, tid);
            }
        }
    if (region) munmap(region, region_len);
    return 0;
}

uint32_t mel_sim_lds_floats(void) { return kLdsFloats; }

}  // extern "C"
